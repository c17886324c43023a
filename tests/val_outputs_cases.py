"""Seeded inputs of the output writers (yolov3_amd.outputs, y3_export_rows): shared by the fixture generator tests/golden/make_val_outputs_golden.py (which runs the
unmodified reference on them) and by tests/test_val_outputs_cpu.py / tests/test_gpu_val_outputs.py (which regenerate them and compare).
Test infrastructure: CPU generators only, nothing here is imported by the product."""
from __future__ import annotations

import torch

SIZES = [(375, 500), (1080, 1919), (480, 640), (427, 640), (333, 500)]   # native (h0, w0): non-square, the divisions are inexact
NAMES = [f"class{i}" for i in range(80)]
TIMES = (0.03125, 0.5, 0.0625)        # seconds per stage (exact in binary: the ms / image of the speed line do not depend on the order of the operations)
DETECTIONS_SHAPE = (3, 3, 640, 640)
# The reference imports coco80_to_coco91_class from a package it does not vendor (utils/general.py:32), so there is no list of its own to record: the map is stated here from
# the COCO paper's numbering -- ids 1 ... 90, of which these ten never got annotations -- and the product's function is compared with it.
COCO_UNUSED_IDS = (12, 26, 29, 30, 45, 66, 68, 69, 71, 83)
COCO_SPOT_CHECKS = {0: 1, 10: 11, 11: 13, 24: 27, 25: 28, 26: 31, 39: 44, 40: 46, 60: 67, 61: 70, 62: 72, 72: 82, 73: 84, 79: 90}   # class index -> category id

_WIDE_COUNTS = [(i * 7 + 3) % 5 if i % 9 else 0 for i in range(70)]   # ragged, with zeros (image 0 among them)
_WIDE_COUNTS[5] = 300                                                 # one full image: count == max_rows
_WIDE_COUNTS[69] = 3

# name -> counts, max_rows, nc; `limits`: the caps the target form is pinned at
CASES = {
    "small": dict(seed=11, counts=[0, 5, 2], max_rows=8, nc=80),                       # a leading empty image: offsets, no file for image 0; COCO class map
    "ids": dict(seed=12, counts=[4, 3], max_rows=5, nc=365, force_cls=364),            # class ids up to 364, identity map
    "wide": dict(seed=13, counts=_WIDE_COUNTS, max_rows=300, nc=365, limits=(300, 7)),  # bs 70: the prefix crosses a wave of images; the cap
    "detect": dict(seed=14, counts=[1, 12, 0, 3], max_rows=12, nc=80, ties=True),       # detect.py's form: exact .5 corners, one row and many rows reversed
}
TXT_CASES = ("small", "ids", "detect")      # cases whose file bytes the golden holds
JSON_CASES = ("small", "ids")               # cases whose jdict the golden holds ("small": COCO map, "ids": identity map)
# corners exactly on k + 0.5, both parities of k: round-half-even gives 10 20 102 202 / 12 22 100 202 / 2 4 44 56 (half away from zero would not)
TIE_BOXES = [(10.5, 20.5, 101.5, 202.5), (11.5, 21.5, 100.5, 201.5), (2.5, 3.5, 44.25, 55.75)]


def coco_map():
    return [i for i in range(1, 91) if i not in COCO_UNUSED_IDS]


def stems(n):
    """numeric (COCO style: image_id is the int) and non-numeric stems"""
    return [f"{139 + 37 * i:012d}" if i % 2 == 0 else f"street_{i}" for i in range(n)]


def case(name):
    """dict(rows (bs, max_rows, 6) fp32 padded [x1, y1, x2, y2, conf, cls] in native pixels, counts, shapes [(h0, w0)], paths, nc).  Rows past an image's count hold -7:
    an export that reads them shows."""
    c = CASES[name]
    g = torch.Generator().manual_seed(c["seed"])
    counts, max_rows, nc = list(c["counts"]), c["max_rows"], c["nc"]
    bs = len(counts)
    shapes = [SIZES[i % len(SIZES)] for i in range(bs)]
    rows = torch.full((bs, max_rows, 6), -7.0)
    for i, n in enumerate(counts):
        if n == 0:
            continue
        h0, w0 = shapes[i]
        u = torch.rand(n, 6, generator=g)
        x1, y1 = u[:, 0] * 0.4 * w0, u[:, 1] * 0.4 * h0
        x2, y2 = x1 + (0.05 + 0.5 * u[:, 2]) * w0, y1 + (0.05 + 0.5 * u[:, 3]) * h0      # fractional corners inside the image
        conf = torch.sort(10.0 ** (-5.0 * u[:, 4]), descending=True).values             # 1e-5 ... 1: %g takes both of its forms
        cls = torch.randint(0, nc, (n,), generator=g).float()
        rows[i, :n] = torch.stack((x1, y1, x2, y2, conf, cls), 1)
    if c.get("force_cls") is not None:
        rows[0, 0, 5] = float(c["force_cls"])
    if c.get("ties"):
        for k, box in enumerate(TIE_BOXES):
            rows[1, k, :4] = torch.tensor(box)
        rows[1, 0, 5] = rows[1, 1, 5]    # two rows of one class: the plural of the class strings
    return dict(rows=rows, counts=counts, shapes=shapes, paths=[f"/data/images/{s}.jpg" for s in stems(bs)], nc=nc, limits=c.get("limits", ()))


def dets(c):
    """the per-image (n, 6) list the reference's loops take"""
    return [c["rows"][i, :n].clone() for i, n in enumerate(c["counts"])]


def checksum(c):
    return float(c["rows"].double().sum())


def as_view(rows, pad_rows=2, row_stride=7):
    """the same rows inside a larger buffer: row stride 7 and an image stride beyond max_rows * row_stride (the buffer's other elements hold 9e9)"""
    bs, m, _ = rows.shape
    buf = torch.full((bs, m + pad_rows, row_stride), 9e9, dtype=rows.dtype, device=rows.device)
    buf[:, :m, :6] = rows
    return buf[:, :m, :6]
