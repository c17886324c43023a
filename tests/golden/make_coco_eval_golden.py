"""Record tests/golden/coco_eval.pt: the fixture scene of tests/coco_eval_cases.py with the arrays its restatement of pycocotools' COCOeval computes (whole), and for
every seeded scene the twelve stats and a SHA-256 of each array (the arrays are recomputed where they are needed; the digests catch a drift of the generators or of
the restatement).  Where pycocotools imports, every array is asserted equal to COCOeval's first.

    python tests/golden/make_coco_eval_golden.py
"""
import hashlib
import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT / "tests"))

import coco_eval_cases as cc  # noqa: E402


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype=np.float64).tobytes()).hexdigest()


def pycocotools_arrays(anno, dets, img_ids):
    """COCOeval's own arrays, or None where pycocotools is not installed"""
    try:
        from pycocotools.coco import COCO
        from pycocotools.cocoeval import COCOeval
    except ImportError:
        return None
    import copy
    import contextlib
    import io

    with contextlib.redirect_stdout(io.StringIO()):
        gt = COCO()
        gt.dataset = copy.deepcopy(anno)
        gt.createIndex()
        known = {c["id"] for c in anno["categories"]}
        dt = gt.loadRes([d for d in copy.deepcopy(dets) if d["category_id"] in known]) if dets else COCO()
        ev = COCOeval(gt, dt, "bbox")
        if img_ids is not None:
            ev.params.imgIds = sorted(set(img_ids))
        ev.evaluate()
        ev.accumulate()
        ev.summarize()
    return ev.eval["precision"], ev.eval["recall"], ev.eval["scores"], ev.stats


def run(anno, dets, img_ids):
    r = cc.evaluate(anno, dets, img_ids)
    theirs = pycocotools_arrays(anno, dets, img_ids)
    if theirs is not None:
        assert np.array_equal(r["precision"], theirs[0]) and np.array_equal(r["recall"], theirs[1]) and np.array_equal(r["scores"], theirs[2])
        assert np.array_equal(r["stats"], theirs[3])
    return r


def main():
    anno, dets = cc.fixture_scene()
    r = run(anno, dets, None)
    out = {"fixture": {"anno": json.dumps(anno), "dets": json.dumps(dets), "precision": torch.from_numpy(r["precision"]), "recall": torch.from_numpy(r["recall"]),
                       "scores": torch.from_numpy(r["scores"]), "stats": torch.from_numpy(r["stats"]), "lines": cc.summarize(r["precision"], r["recall"])[1]},
           "scenes": {}, "pycocotools": pycocotools_arrays(anno, dets, None) is not None}
    for name in cc.SCENES:
        anno, dets, img_ids = cc.scene(name)
        r = run(anno, dets, img_ids)
        out["scenes"][name] = {"stats": torch.from_numpy(r["stats"]), "n_gt": len(anno["annotations"]), "n_det": len(dets),
                               "sha256": {k: digest(r[k]) for k in ("precision", "recall", "scores")}}
    torch.save(out, ROOT / "tests" / "golden" / "coco_eval.pt")
    print({k: (v["n_gt"], v["n_det"]) for k, v in out["scenes"].items()}, "pycocotools:", out["pycocotools"])


if __name__ == "__main__":
    main()
