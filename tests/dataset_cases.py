"""Shared inputs of the device-resident dataset tests (tests/test_dataset_cpu.py, tests/test_gpu_dataset.py, tests/golden/make_dataset_golden.py): eight seeded
cached images, their labels and the cases.  Not a test file.

img_size 64, stride 32, batch size 3: the smallest set at which every branch of the layout and of the kernels is taken --
  * file order D E G C H F A B, aspect-ratio order A B C | D E F | G H: a wide-only, a mixed and a tall-only batch, the last one partial;
  * D is 37 x 61 (h x w): a width that is no multiple of 4, so its source rows start at every byte alignment, and paddings whose halves differ (dw = 17.5 / 1.5,
    dh = 29.5 / 13.5: left != right, top != bottom); H is 64 x 23: dw = 20.5;
  * E is 64 x 64: no border at all in a 64 x 64 batch (rect with pad 0, and rect=False), where its labels touch and cross the border, so that the eps clip acts;
  * B has no labels inside a batch that has some; G and H have none: a batch with no labels at all; zero-area labels on D and E;
  * batch widths 64 and 96, heights 32, 64 and 96; several blocks per batch.
"""
from __future__ import annotations

import zlib

import numpy as np

IMG_SIZE, STRIDE, BATCH = 64, 32, 3

# file stem, cached (h, w), original (h0, w0) -- in file order, which is the order the constructor gets them in
IMAGES = [
    ("000001", (37, 61), (259, 427)),   # D  h0 / w0 = 0.607
    ("000002", (64, 64), (448, 448)),   # E  1.0
    ("000003", (64, 41), (640, 410)),   # G  1.561
    ("000004", (30, 64), (211, 450)),   # C  0.469
    ("000005", (64, 23), (500, 180)),   # H  2.778
    ("000006", (64, 50), (512, 400)),   # F  1.28
    ("000007", (16, 64), (120, 480)),   # A  0.25
    ("000008", (21, 64), (157, 480)),   # B  0.327
]
RECT_ORDER = [6, 7, 3, 0, 1, 5, 2, 4]   # what the aspect-ratio sort must give

LABELS = [
    [[3, 0.5, 0.5, 0.4, 0.3], [17, 0.98, 0.5, 0.3, 0.2], [0, 0.02, 0.03, 0.2, 0.2], [5, 0.7, 0.9, 0.0, 0.0]],                                       # D
    [[1, 0.75, 0.5, 0.5, 0.5], [2, 0.98, 0.96, 0.3, 0.3], [79, 0.01, 0.5, 0.1, 1.0], [4, 0.5, 0.5, 0.0, 0.0], [7, 1.0, 1.0, 0.0, 0.0],
     [22, 0.3337, 0.6113, 0.2471, 0.1234]],                                                                                                     # E
    [],                                                                                                                                         # G
    [[9, 0.3, 0.4, 0.2, 0.5], [9, 0.99, 0.5, 0.02, 1.0]],                                                                                       # C
    [],                                                                                                                                         # H
    None,                                                                                                                                       # F: seeded below
    [[11, 0.5, 0.5, 1.0, 1.0]],                                                                                                                 # A
    [],                                                                                                                                         # B
]

# name -> the constructor's arguments; `indices`: the epoch's order of a rect=False set (set_indices)
CASES = {
    "rect_pad05": dict(rect=True, pad=0.5, single_cls=False, indices=None),
    "rect_pad00": dict(rect=True, pad=0.0, single_cls=False, indices=None),
    "square": dict(rect=False, pad=0.0, single_cls=False, indices=None),
    "square_perm": dict(rect=False, pad=0.0, single_cls=False, indices=[int(i) for i in np.random.RandomState(7).permutation(len(IMAGES))]),
    "rect_single_cls": dict(rect=True, pad=0.5, single_cls=True, indices=None),
}
# the cases whose letterboxed images are, image for image, those of another case: the fixture stores them once
IMAGES_OF = {"square_perm": "square", "rect_single_cls": "rect_pad05"}


def _rng(what: str) -> np.random.RandomState:
    return np.random.RandomState(zlib.crc32(f"dataset:{what}".encode()))


def paths() -> list:
    return [f"images/{stem}.png" for stem, _, _ in IMAGES]


def make_images() -> list:
    """the cached images, (h, w, 3) uint8 BGR, seeded noise: every byte matters"""
    return [_rng(stem).randint(0, 256, (h, w, 3)).astype(np.uint8) for stem, (h, w), _ in IMAGES]


def make_labels() -> list:
    """dataset.labels in file order: (m, 5) float32 [class, x, y, w, h], all inside [0, 1] and free of duplicates (what the reference's label check accepts)"""
    out = []
    for (stem, _, _), rows in zip(IMAGES, LABELS):
        if rows is None:
            rs = _rng("labels:" + stem)
            rows = np.concatenate([rs.randint(0, 80, (3, 1)).astype(np.float64), rs.uniform(0.2, 0.8, (3, 2)), rs.uniform(0.05, 0.4, (3, 2))], 1)
        out.append(np.array(rows, dtype=np.float32).reshape(-1, 5))
    return out


def hw() -> list:
    return [s for _, s, _ in IMAGES]


def hw0() -> list:
    return [s for _, _, s in IMAGES]


def checksum(images, labels) -> float:
    return float(sum(int(im.astype(np.int64).sum()) for im in images) + sum(float(l.astype(np.float64).sum()) + 3.0 * len(l) for l in labels))


def expected_images(gold, case: str, k: int):
    """the uint8 batch k of `case` from the fixture (stored, or stacked from the case that holds the same letterboxed images)"""
    import torch

    b = gold["cases"][case]["batches"][k]
    if "im" in b:
        return b["im"]
    src = gold["cases"][IMAGES_OF[case]]["batches"]
    return torch.stack([src[bk]["im"][slot] for bk, slot in b["im_from"]], 0)
