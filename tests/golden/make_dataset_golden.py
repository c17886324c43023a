"""Generate tests/golden/dataset.pt from the UNMODIFIED reference: utils.dataloaders.LoadImagesAndLabels (through oracle/ref_shim.py) -- its real __init__ for the
aspect-ratio order, `batch` and `batch_shapes`, its real __getitem__ and collate_fn for every batch of every case of tests/dataset_cases.py.

    python tests/golden/make_dataset_golden.py

Only where the reference tree is present.  The file holds tensors, tuples, numbers and names only.

How the reference is driven without cv2 and without the ultralytics package (both are stubs under the shim):
  * __init__ runs on a temporary directory of blank PNGs of the ORIGINAL sizes (written with PIL) and the label files; cache_images stays off, and the seeded
    cached images are placed in .ims / .im_hw0 / .im_hw afterwards, as `--cache ram` leaves them;
  * cv2.copyMakeBorder of the stub becomes a constant np.pad -- the pad-only branch of letterbox calls nothing else from cv2 (a cv2.resize call would fail loudly);
  * the names utils.dataloaders imports from the ultralytics package are bound HERE to restatements of their published definitions, written for this file:
      xywhn2xyxy, xyxy2xywhn (and the NumPy branch of clip_boxes inside it) -- THE LABEL EXPECTATIONS REST ON THESE RESTATEMENTS, the images on the reference alone;
      img2label_paths ("/images/" -> "/labels/", ".txt"), get_hash (any stable value serves a fresh cache) and a TQDM that only iterates.
"""
import os
import sys
import tempfile
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import dataset_cases as dc  # noqa: E402
from oracle import ref_shim  # noqa: E402


def xywhn2xyxy(x, w=640, h=640, padw=0, padh=0):
    """normalised [x, y, w, h] -> pixel [x1, y1, x2, y2] of an image of (w, h) placed at (padw, padh)"""
    y = np.empty_like(x)
    xc, yc, xw, xh = x[..., 0], x[..., 1], x[..., 2], x[..., 3]
    half_w, half_h = xw / 2, xh / 2
    y[..., 0] = w * (xc - half_w) + padw
    y[..., 1] = h * (yc - half_h) + padh
    y[..., 2] = w * (xc + half_w) + padw
    y[..., 3] = h * (yc + half_h) + padh
    return y


def xyxy2xywhn(x, w=640, h=640, clip=False, eps=0.0):
    """pixel [x1, y1, x2, y2] -> normalised [x, y, w, h], clipped to (h - eps, w - eps) first"""
    if clip:
        x[..., [0, 2]] = x[..., [0, 2]].clip(0, w - eps)
        x[..., [1, 3]] = x[..., [1, 3]].clip(0, h - eps)
    y = np.empty_like(x)
    x1, y1, x2, y2 = x[..., 0], x[..., 1], x[..., 2], x[..., 3]
    y[..., 0] = ((x1 + x2) / 2) / w
    y[..., 1] = ((y1 + y2) / 2) / h
    y[..., 2] = (x2 - x1) / w
    y[..., 3] = (y2 - y1) / h
    return y


def img2label_paths(img_paths):
    sa, sb = f"{os.sep}images{os.sep}", f"{os.sep}labels{os.sep}"
    return [sb.join(x.rsplit(sa, 1)).rsplit(".", 1)[0] + ".txt" for x in img_paths]


class _Progress:
    def __init__(self, iterable=None, **kw):
        self.iterable, self.desc = iterable, ""

    def __iter__(self):
        return iter(self.iterable)

    def close(self):
        pass


def copy_make_border(im, top, bottom, left, right, border_type, value=(0, 0, 0)):
    assert len(set(value)) == 1
    return np.pad(im, ((top, bottom), (left, right), (0, 0)), mode="constant", constant_values=value[0])


def reference():
    ref_shim.install()
    import cv2  # the shim's stub
    import utils.dataloaders as d  # type: ignore

    cv2.copyMakeBorder = copy_make_border
    d.xywhn2xyxy, d.xyxy2xywhn, d.img2label_paths, d.get_hash, d.TQDM = xywhn2xyxy, xyxy2xywhn, img2label_paths, (lambda paths: "dataset-golden"), _Progress
    return d


def write_tree(root: Path):
    """blank PNGs of the original sizes and the label files, in the layout the reference's __init__ reads"""
    from PIL import Image

    (root / "images").mkdir()
    (root / "labels").mkdir()
    for (stem, _, (h0, w0)), lb in zip(dc.IMAGES, dc.make_labels()):
        Image.new("RGB", (w0, h0), (90, 120, 150)).save(root / "images" / f"{stem}.png")
        (root / "labels" / f"{stem}.txt").write_text("".join(" ".join([str(int(r[0]))] + [repr(float(v)) for v in r[1:]]) + "\n" for r in lb))


def build_dataset(d, root: Path, case: str):
    """the reference dataset of one case, its cache filled by hand, its file names made relative"""
    c = dc.CASES[case]
    ds = d.LoadImagesAndLabels(str(root / "images"), img_size=dc.IMG_SIZE, batch_size=dc.BATCH, augment=False, rect=c["rect"], cache_images=False,
                               single_cls=c["single_cls"], stride=dc.STRIDE, pad=c["pad"])
    stems = [Path(f).stem for f in ds.im_files]
    file_index = [[s for s, _, _ in dc.IMAGES].index(s) for s in stems]   # dataset position -> file-order position
    images, labels = dc.make_images(), dc.make_labels()
    for j, i in enumerate(file_index):
        want = labels[i].copy()
        if c["single_cls"]:
            want[:, 0] = 0
        assert ds.labels[j].dtype == np.float32 and np.array_equal(ds.labels[j], want), f"{case}: the labels of {stems[j]} did not survive the label files"
        assert tuple(ds.shapes[j]) == dc.IMAGES[i][2][::-1]
    ds.ims = [images[i] for i in file_index]
    ds.im_hw0 = [dc.IMAGES[i][2] for i in file_index]
    ds.im_hw = [dc.IMAGES[i][1] for i in file_index]
    ds.im_files = [dc.paths()[i] for i in file_index]
    if c["indices"] is not None:
        ds.indices = list(c["indices"])
    return ds, file_index


def plain(v):
    """tuples of Python numbers"""
    return tuple(plain(x) for x in v) if isinstance(v, (tuple, list, np.ndarray)) else (float(v) if isinstance(v, (float, np.floating)) else int(v))


def run_case(d, root: Path, case: str, stored: dict):
    ds, file_index = build_dataset(d, root, case)
    n = len(ds.im_files)
    out = dict(order=torch.tensor(file_index), batch=torch.from_numpy(np.asarray(ds.batch).astype(np.int64)), paths=list(ds.im_files))
    if ds.rect:
        out["batch_shapes"] = torch.from_numpy(ds.batch_shapes.astype(np.int64))
    batches = []
    for k in range((n + dc.BATCH - 1) // dc.BATCH):
        im, targets, paths, shapes = d.LoadImagesAndLabels.collate_fn([ds[i] for i in range(k * dc.BATCH, min(n, (k + 1) * dc.BATCH))])
        assert im.dtype == torch.uint8 and targets.dtype == torch.float32
        b = dict(targets=targets.clone(), paths=list(paths), shapes=plain(shapes))
        if case in dc.IMAGES_OF:   # the same letterboxed images as another case's: checked here, stored there
            src = stored[dc.IMAGES_OF[case]]["batches"]
            where = [divmod(ds.indices[i], dc.BATCH) for i in range(k * dc.BATCH, min(n, (k + 1) * dc.BATCH))]
            assert torch.equal(im, torch.stack([src[bk]["im"][slot] for bk, slot in where], 0))
            b["im_from"] = [(int(bk), int(slot)) for bk, slot in where]
        else:
            b["im"] = im.clone()
        batches.append(b)
    out["batches"] = batches
    return out


def main():
    d = reference()
    images, labels = dc.make_images(), dc.make_labels()
    gold = {"meta": {"numpy": np.__version__, "torch": str(torch.__version__), "python": sys.version.split()[0]}, "checksum": dc.checksum(images, labels), "cases": {}}
    for case in dc.CASES:
        with tempfile.TemporaryDirectory() as tmp:   # (a fresh tree per case: the label cache of one case is not read by the next)
            write_tree(Path(tmp))
            gold["cases"][case] = run_case(d, Path(tmp), case, gold["cases"])
        print(case, [tuple(b["im"].shape) if "im" in b else b["im_from"] for b in gold["cases"][case]["batches"]], [len(b["targets"]) for b in gold["cases"][case]["batches"]])
    path = ROOT / "tests" / "golden" / "dataset.pt"
    torch.save(gold, path)
    torch.load(path, weights_only=True)   # data only: tensors, numbers, strings
    print(path, path.stat().st_size, "bytes", gold["meta"])


if __name__ == "__main__":
    main()
