"""Shared inputs of the train-mode dataset tests (tests/test_augment_cpu.py, tests/test_gpu_augment.py, tests/golden/make_augment_golden.py): twelve seeded cached
images, their labels, the cases -- and the two definitions the images rest on where cv2 itself would decide: the 8-bit INTER_LINEAR sampler of cv2.warpAffine and the
two 8-bit cv2.cvtColor conversions (BGR <-> HSV, H in [0, 180)), written once, as NumPy.  Not a test file.

NEITHER STATEMENT HAS BEEN COMPARED WITH A cv2 BUILD (none is on the build machine): they restate the published algorithms, and csrc/augment.hip must match them bit
for bit.  The case `exact` does not depend on them: its warp is a translation by whole pixels (asserted by the generator to equal the plain crop) and its HSV gains are 0.

img_size 64, batch 4: twelve images with a long side of exactly 64 (what load_image leaves for img_size 64), odd widths so that arena rows start at odd bytes, 0 .. 6
labels each, one image without labels.
"""
from __future__ import annotations

import math
import zlib

import numpy as np

IMG_SIZE, STRIDE, BATCH = 64, 32, 4

# file stem, cached (h, w), original (h0, w0)
IMAGES = [
    ("000001", (64, 48), (640, 480)),
    ("000002", (37, 64), (370, 640)),
    ("000003", (64, 64), (500, 500)),
    ("000004", (64, 23), (512, 184)),
    ("000005", (51, 64), (408, 512)),
    ("000006", (64, 61), (640, 610)),
    ("000007", (16, 64), (120, 480)),
    ("000008", (64, 41), (640, 410)),
    ("000009", (45, 64), (360, 512)),
    ("000010", (64, 57), (448, 399)),
    ("000011", (30, 64), (211, 450)),
    ("000012", (64, 33), (620, 320)),
]
LABEL_COUNTS = [3, 5, 6, 1, 4, 2, 0, 3, 6, 2, 1, 4]

_BASE = dict(mosaic=1.0, degrees=0.0, translate=0.0, scale=0.0, shear=0.0, perspective=0.0, hsv_h=0.0, hsv_s=0.0, hsv_v=0.0, flipud=0.0, fliplr=0.0, mixup=0.0, copy_paste=0.0)
_LOW = dict(_BASE, translate=0.1, scale=0.5, hsv_h=0.015, hsv_s=0.7, hsv_v=0.4, fliplr=0.5)   # the augmentation values of data/hyps/hyp.scratch-low.yaml

# name -> hyp, the seeds of `random` / `np.random` for the epoch, the epoch's order (`indices`, None: range(n)) and the output dtype
CASES = {
    "exact": dict(hyp=dict(_BASE, flipud=0.5, fliplr=0.5, mixup=0.5), seed=0, indices=None, dtype="uint8"),
    "low": dict(hyp=dict(_LOW), seed=0, indices=None, dtype="uint8"),
    "wild": dict(hyp=dict(_BASE, degrees=10.0, translate=0.2, scale=0.9, shear=5.0, hsv_h=0.015, hsv_s=0.7, hsv_v=0.4, flipud=0.5, fliplr=0.5, mixup=0.3), seed=0,
                 indices=[int(i) for i in np.random.RandomState(11).permutation(len(IMAGES))] + [5, 5, 2, 5], dtype="uint8"),   # a shuffle, then a draw that repeats
    "single": dict(hyp=dict(_BASE, mosaic=0.0, translate=0.1, scale=0.5, hsv_h=0.015, hsv_s=0.7, hsv_v=0.4, fliplr=0.5), seed=0, indices=None, dtype="uint8"),
    "low_f16": dict(hyp=dict(_LOW), seed=0, indices=None, dtype="float16"),
}
IMAGES_OF = {"low_f16": "low"}   # the same uint8 batches as another case's: stored once


def _rng(what: str) -> np.random.RandomState:
    return np.random.RandomState(zlib.crc32(f"augment:{what}".encode()))


def paths() -> list:
    return [f"images/{stem}.png" for stem, _, _ in IMAGES]


def hw() -> list:
    return [s for _, s, _ in IMAGES]


def hw0() -> list:
    return [s for _, _, s in IMAGES]


def make_images() -> list:
    """the cached images, (h, w, 3) uint8 BGR: smooth colour ramps plus noise, so that HSV sees every hue and the sampler every byte"""
    out = []
    for stem, (h, w), _ in IMAGES:
        rs = _rng(stem)
        y, x = np.mgrid[0:h, 0:w]
        base = np.stack([(x * rs.randint(2, 9) + y * rs.randint(1, 5) + rs.randint(0, 256)) % 256 for _ in range(3)], -1)
        noise = rs.randint(0, 256, (h, w, 3))
        out.append(np.where(rs.uniform(size=(h, w, 1)) < 0.5, base, noise).astype(np.uint8))
    return out


def make_labels() -> list:
    """dataset.labels: (m, 5) float32 [class, x, y, w, h], inside [0, 1], free of duplicates; small and large boxes, some touching the image edge"""
    out = []
    for (stem, _, _), m in zip(IMAGES, LABEL_COUNTS):
        rs = _rng("labels:" + stem)
        wh = rs.uniform(0.03, 0.6, (m, 2))
        c = rs.uniform(0.0, 1.0, (m, 2)) * (1 - wh) + wh / 2   # the box lies inside the image
        rows = np.concatenate([rs.randint(0, 80, (m, 1)).astype(np.float64), c, wh], 1)
        out.append(np.array([[float(f"{v:.6f}") for v in r] for r in rows], dtype=np.float32).reshape(-1, 5))
    return out


def checksum(images, labels) -> float:
    return float(sum(int(im.astype(np.int64).sum()) for im in images) + sum(float(l.astype(np.float64).sum()) + 3.0 * len(l) for l in labels))


def expected_images(gold, case: str, k: int):
    """the uint8 batch k of `case` from the fixture"""
    return gold["cases"][IMAGES_OF.get(case, case)]["batches"][k]["im"]


# ---- cv2.getRotationMatrix2D, restated from its documented formula ---------------------------------------------------------------------------------------------------
def get_rotation_matrix_2d(angle, center, scale):
    a = angle * math.pi / 180
    alpha, beta = math.cos(a) * scale, math.sin(a) * scale
    cx, cy = center
    return np.array([[alpha, beta, (1 - alpha) * cx - beta * cy], [-beta, alpha, beta * cx + (1 - alpha) * cy]], dtype=np.float64)


# ---- the sampler: cv2.warpAffine(src, M, dsize, flags=INTER_LINEAR, borderMode=BORDER_CONSTANT) on 8-bit images ---------------------------------------------------------
AB_SCALE = 1024      # 1 << max(10, INTER_BITS)
ROUND_DELTA = 16     # AB_SCALE / INTER_TAB_SIZE / 2 with INTER_TAB_SIZE = 32


def invert_affine(M):
    """cv2.invertAffineTransform in float64 -> the six numbers (A00, A01, A02, A10, A11, A12) as Python floats"""
    m00, m01, m02, m10, m11, m12 = (float(v) for v in np.asarray(M, dtype=np.float64)[:2].reshape(-1))
    D = m00 * m11 - m01 * m10
    D = 1.0 / D if D != 0 else 0.0
    a00, a11 = m11 * D, m00 * D
    a01, a10 = m01 * -D, m10 * -D
    return a00, a01, -a00 * m02 - a01 * m12, a10, a11, -a10 * m02 - a11 * m12


def warp_coordinates(M, width, height):
    """the source coordinate of every output pixel in 1 / 32 pixel: int64 (height, width) X and Y"""
    a00, a01, a02, a10, a11, a12 = invert_affine(M)
    x, y = np.arange(width, dtype=np.float64), np.arange(height, dtype=np.float64)[:, None]
    X = (np.rint((a01 * y + a02) * AB_SCALE).astype(np.int64) + ROUND_DELTA + np.rint(a00 * x * AB_SCALE).astype(np.int64)) >> 5
    Y = (np.rint((a11 * y + a12) * AB_SCALE).astype(np.int64) + ROUND_DELTA + np.rint(a10 * x * AB_SCALE).astype(np.int64)) >> 5
    return X, Y


def warp_affine_u8(src, M, dsize, border=114):
    """src (h, w, c) uint8, M the forward 2 x 3 matrix, dsize (width, height) -> (height, width, c) uint8.  Five fractional bits; the four taps are weighted by
    (32 - fy | fy) (32 - fx | fx), summed as integers, + 512 >> 10 (the published 15-bit table holds exactly these products times 32); a tap outside src is `border`."""
    width, height = dsize
    X, Y = warp_coordinates(M, width, height)
    sx, sy, fx, fy = X >> 5, Y >> 5, X & 31, Y & 31
    h, w = src.shape[:2]
    acc = np.zeros((height, width, src.shape[2]), dtype=np.int64)
    for dy, wy in ((0, 32 - fy), (1, fy)):
        for dx, wx in ((0, 32 - fx), (1, fx)):
            tx, ty = sx + dx, sy + dy
            inside = (tx >= 0) & (tx < w) & (ty >= 0) & (ty < h)
            p = np.where(inside[..., None], src[np.clip(ty, 0, h - 1), np.clip(tx, 0, w - 1)].astype(np.int64), border)
            acc += (wy * wx)[..., None] * p
    return ((acc + 512) >> 10).astype(np.uint8)


# ---- the colour conversions: cv2.cvtColor(COLOR_BGR2HSV / COLOR_HSV2BGR) on 8-bit images, H in [0, 180) ----------------------------------------------------------------
HSV_SHIFT = 12
_SDIV = np.array([0] + [int(np.rint((255 << HSV_SHIFT) / (1.0 * i))) for i in range(1, 256)], dtype=np.int64)
_HDIV = np.array([0] + [int(np.rint((180 << HSV_SHIFT) / (6.0 * i))) for i in range(1, 256)], dtype=np.int64)


def bgr2hsv_u8(im):
    """integer throughout: s = (diff sdiv[v] + 2^11) >> 12, h = (h' hdiv[diff] + 2^11) >> 12 (+ 180 below zero)"""
    b, g, r = (im[..., c].astype(np.int64) for c in range(3))
    v = np.maximum(np.maximum(b, g), r)
    diff = v - np.minimum(np.minimum(b, g), r)
    s = (diff * _SDIV[v] + (1 << (HSV_SHIFT - 1))) >> HSV_SHIFT
    h = np.where(v == r, g - b, np.where(v == g, b - r + 2 * diff, r - g + 4 * diff))
    h = (h * _HDIV[diff] + (1 << (HSV_SHIFT - 1))) >> HSV_SHIFT
    h = h + np.where(h < 0, 180, 0)
    return np.stack([np.clip(h, 0, 255), s, v], -1).astype(np.uint8)


_SECTOR = np.array([[1, 3, 0], [1, 0, 2], [3, 0, 1], [0, 2, 1], [0, 1, 3], [2, 1, 0]])   # which of the four products is b, g, r in sector 0 .. 5


def hsv2bgr_u8(im):
    """fp32, every operation rounded on its own, in this order: s = S * (1 / 255), v = V * (1 / 255), h = H * (6 / 180); sector = floor(h), f = h - sector;
    the products v, v (1 - s), v (1 - s f), v (1 - s (1 - f)); the sector table; * 255, rounded half to even, saturated.  s == 0: b = g = r = v."""
    f32 = np.float32
    one, k255 = f32(1.0), f32(1.0) / f32(255.0)
    h = im[..., 0].astype(f32) * (f32(6.0) / f32(180.0))
    s = im[..., 1].astype(f32) * k255
    v = im[..., 2].astype(f32) * k255
    sector = np.floor(h)
    f = h - sector
    sector = sector.astype(np.int64)
    bad = (sector < 0) | (sector >= 6)
    sector, f = np.where(bad, 0, sector), np.where(bad, f32(0.0), f)
    tab = np.stack([v, v * (one - s), v * (one - s * f), v * (one - s * (one - f))], -1)
    assert tab.dtype == f32
    bgr = np.take_along_axis(tab, _SECTOR[sector], -1)
    bgr = np.where((im[..., 1] == 0)[..., None], v[..., None], bgr)
    return np.clip(np.rint(bgr * f32(255.0)), 0, 255).astype(np.uint8)
