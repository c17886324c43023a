"""Generate tests/golden/classifier_crops.pt from the UNMODIFIED reference: utils.general.apply_classifier (through oracle/ref_shim.py) on the case of
tests/classifier_crops_cases.py.

    python tests/golden/make_classifier_crops_golden.py

Only where the reference tree is present.  The file holds tensors, numbers and strings only.

How the reference is driven without cv2 (a stub under the shim): cv2.resize is bound HERE to a recorder that keeps the cutout it is handed and answers with
oracle.yolo_oracle.resize_linear_u8 -- the 8-bit INTER_LINEAR restatement that backs y3_letterbox_u8 and that no cv2 build has checked.  Everything else --
xyxy2xywh, the square, the pad, xywh2xyxy, .long(), scale_boxes with clip_boxes, the slicing, the channel flip, the transpose, the float conversion, `/= 255`, the
classifier call per image and the filter -- is the reference's own code.  What is asserted before anything is written:
  * every cutout the reference cut equals the statement's, and it cut as many as there are detections;
  * the classifier's recorded inputs equal the statement's crops, and every crop times 255 round-trips to the uint8 the resize returned;
  * the rows the reference kept equal the statement's;
  * check_situations: the case reaches every situation it exists for.
The fixture holds the images, the detections, the boxes, the predicted classes, the kept rows, two crops whole (uint8) and a SHA-256 of every crop; the tests
recompute the crops from the statement.
"""
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import classifier_crops_cases as cc  # noqa: E402
from oracle import ref_shim  # noqa: E402
from oracle.yolo_oracle import resize_linear_u8  # noqa: E402


def main():
    ref_shim.install()
    import cv2  # the shim's stub
    import utils.general as g  # type: ignore

    recorded = []

    def resize(src, dsize, *a, **k):
        assert not a and not k and tuple(dsize) == (cc.SIZE, cc.SIZE)
        recorded.append(np.array(src, copy=True))
        return resize_linear_u8(src, dsize[0], dsize[1])

    cv2.resize = resize
    g.cv2.resize = resize
    ims, x = cc.build_case()
    st = cc.statement(ims, x)
    cc.check_situations(ims, x, st)

    model = cc.ToyClassifier()
    out = g.apply_classifier([None if d is None else d.clone() for d in x], model, torch.zeros(1, 3, *cc.IMG1), ims)

    live = [i for i, d in enumerate(x) if d is not None and len(d)]
    want_cut = [c for i in live for c in cc.cutouts(ims[i], st["boxes"][i])]
    assert len(recorded) == len(want_cut) == sum(len(x[i]) for i in live)
    for a, b in zip(recorded, want_cut):
        assert a.shape == b.shape and np.array_equal(a, b)
    assert len(model.seen) == len(live)
    for i, seen in zip(live, model.seen):
        want = cc.to_float(st["crops"][i])
        assert seen.dtype == torch.float32 and torch.equal(seen, want)
        back = (seen * 255).round().to(torch.uint8).numpy()[:, ::-1].transpose(0, 2, 3, 1)
        assert np.array_equal(back, st["crops"][i]) and torch.equal(torch.from_numpy(np.ascontiguousarray(back[..., ::-1].transpose(0, 3, 1, 2))).float() / 255, seen)
    for i, d in enumerate(x):
        if d is None:
            assert out[i] is None
        elif not len(d):
            assert out[i].shape == (0, 6)
        else:
            assert torch.equal(out[i], st["kept"][i])

    gold = {
        "meta": {"numpy": np.__version__, "torch": str(torch.__version__), "python": sys.version.split()[0]},
        "img1": cc.IMG1, "size": cc.SIZE,
        "images": [torch.from_numpy(im.copy()) for im in ims],
        "x": [None if d is None else d.clone() for d in x],
        "boxes": [None if b is None else b.clone() for b in st["boxes"]],
        "pred": [None if p is None else p.clone() for p in st["pred"]],
        "kept": [None if k is None else k.clone() for k in st["kept"]],
        "sha": [None if c is None else [cc.sha(t) for t in c] for c in st["crops"]],
        "full": {f"{i},{j}": torch.from_numpy(st["crops"][i][j].copy()) for i, j in cc.FULL_CROPS},
    }
    path = ROOT / "tests" / "golden" / "classifier_crops.pt"
    torch.save(gold, path)
    torch.load(path, weights_only=True)   # data only
    print(path, path.stat().st_size, "bytes", gold["meta"], [0 if d is None else len(d) for d in x], [0 if k is None else len(k) for k in st["kept"]])


if __name__ == "__main__":
    main()
