"""Shared inputs of the rect train-mode dataset tests (tests/test_augment_rect_cpu.py, tests/test_gpu_augment_rect.py, tests/golden/make_augment_rect_golden.py): the
cases over the twelve images of tests/augment_cases.py with stride 16 -- three batches of four in aspect-ratio order, shaped (48, 64), (64, 64) and (64, 48) -- and
the NumPy statement of one rect item: the letterbox paste, warp_affine_u8, the HSV tables between bgr2hsv_u8 and hsv2bgr_u8, the flips, CHW / RGB for the image, and
xywhn2xyxy, the four corners, the per-axis clip, box_candidates, xyxy2xywhn(clip=True) and the flips for the labels.  The generator asserts both equal to the unmodified
reference item by item.  Not a test file.

With stride 32 every batch shape of these images is 64 x 64, which pins nothing: hence 16."""
from __future__ import annotations

import numpy as np

import augment_cases as ac

IMG_SIZE, STRIDE, BATCH = ac.IMG_SIZE, 16, ac.BATCH

# the set's order (file stems, by h0 / w0 ascending), its batch shapes (H, W) and the letterbox halves (dw, dh) of every image of that order
ORDER = ["000007", "000011", "000002", "000009", "000005", "000003", "000006", "000010", "000001", "000008", "000012", "000004"]
BATCH_SHAPES = [(48, 64), (64, 64), (64, 48)]

_BASE = dict(ac._BASE)
SEED = 0
CASES = {
    "rect_exact": dict(hyp=dict(_BASE, flipud=0.5, fliplr=0.5), seed=SEED, dtype="uint8"),   # M is the identity: the plain letterbox paste
    "rect_low": dict(hyp=dict(ac._LOW), seed=SEED, dtype="uint8"),                            # the augmentation values of data/hyps/hyp.scratch-low.yaml
    "rect_wild": dict(hyp=dict(_BASE, degrees=10.0, translate=0.2, scale=0.9, shear=5.0, hsv_h=0.015, hsv_s=0.7, hsv_v=0.4, flipud=0.5, fliplr=0.5), seed=SEED, dtype="uint8"),
    "rect_low_f16": dict(hyp=dict(ac._LOW), seed=SEED, dtype="float16"),
}
IMAGES_OF = {"rect_low_f16": "rect_low"}   # the same uint8 batches as another case's: stored once


def file_index() -> list:
    """set position -> position in ac.IMAGES"""
    stems = [s for s, _, _ in ac.IMAGES]
    return [stems.index(s) for s in ORDER]


def sorted_set():
    """-> (images, labels, hw, hw0, paths) in the set's order"""
    fi = file_index()
    images, labels, hw, hw0, paths = ac.make_images(), ac.make_labels(), ac.hw(), ac.hw0(), ac.paths()
    return [images[i] for i in fi], [labels[i] for i in fi], [hw[i] for i in fi], [hw0[i] for i in fi], [paths[i] for i in fi]


def expected_images(gold, case: str, k: int):
    """the uint8 batch k of `case` from the fixture"""
    return gold["cases"][IMAGES_OF.get(case, case)]["batches"][k]["im"]


def xywhn2xyxy(x, w, h, padw, padh):
    """The reference's as NumPy (>= 2) evaluates it on the rect path: letterbox takes the batch shape from a NumPy array, so its ratio and halves -- w, h, padw and
    padh here -- are float64 scalars; the product and the sum are float64 and the fp32 label array rounds them once."""
    w, h, padw, padh = np.float64(w), np.float64(h), np.float64(padw), np.float64(padh)
    y = np.copy(x)
    y[..., 0] = w * (x[..., 0] - x[..., 2] / 2) + padw
    y[..., 1] = h * (x[..., 1] - x[..., 3] / 2) + padh
    y[..., 2] = w * (x[..., 0] + x[..., 2] / 2) + padw
    y[..., 3] = h * (x[..., 1] + x[..., 3] / 2) + padh
    return y


def xyxy2xywhn(x, w, h, eps=1e-3):
    """the reference's with clip=True"""
    x = np.copy(x)
    x[..., [0, 2]] = x[..., [0, 2]].clip(0, w - eps)
    x[..., [1, 3]] = x[..., [1, 3]].clip(0, h - eps)
    y = np.copy(x)
    y[..., 0] = ((x[..., 0] + x[..., 2]) / 2) / w
    y[..., 1] = ((x[..., 1] + x[..., 3]) / 2) / h
    y[..., 2] = (x[..., 2] - x[..., 0]) / w
    y[..., 3] = (x[..., 3] - x[..., 1]) / h
    return y


def paste(mo, images, H, W):
    """the letterboxed image of a drawn item: its one tile on an H x W canvas of 114"""
    canvas = np.full((H, W, 3), 114, dtype=np.uint8)
    for j, (x1a, y1a, x2a, y2a, x1b, y1b, x2b, y2b) in zip(mo.indices, mo.rects):
        canvas[y1a:y2a, x1a:x2a] = images[j][y1b:y2b, x1b:x2b]
    return canvas


def item_image(item, images, H, W):
    """one rect item's image as the kernel must write it: (3, H, W) uint8 RGB"""
    mo = item.mosaics[0]
    im = ac.warp_affine_u8(paste(mo, images, H, W), mo.M[:2], (W, H))
    if item.luts is not None:
        hsv = ac.bgr2hsv_u8(im)
        im = ac.hsv2bgr_u8(np.stack([item.luts[c][hsv[..., c]] for c in range(3)], -1))
    if item.flipud:
        im = im[::-1]
    if item.fliplr:
        im = im[:, ::-1]
    return np.ascontiguousarray(im.transpose(2, 0, 1)[::-1])


def item_labels(item, labels, hw, H, W, stats=None, check=False):
    """One rect item's label rows as csrc/augment.hip computes them (fp32 / fp64 as the reference's arrays are, the corner transform a plain left-to-right sum) ->
    (nl, 5) fp32.  stats: collects the situations of the generator's check_situations; check: assert that the BLAS product rounds to the same fp32 boxes and that no
    box_candidates comparison lies within 1e-9 relative of its threshold."""
    mo = item.mosaics[0]
    j, (padw, padh) = mo.indices[0], mo.pad[0]
    t = labels[j].copy()
    if t.size:
        t[:, 1:] = xywhn2xyxy(t[:, 1:], hw[j][1], hw[j][0], padw, padh)
    n = len(t)
    if stats is not None:
        stats["no_labels"] += int(n == 0)
    if n:
        M = mo.M
        p = t[:, [1, 2, 3, 4, 1, 4, 3, 2]].reshape(n * 4, 2).astype(np.float64)
        x = (p[:, 0] * M[0, 0] + p[:, 1] * M[0, 1] + M[0, 2]).reshape(n, 4)
        y = (p[:, 0] * M[1, 0] + p[:, 1] * M[1, 1] + M[1, 2]).reshape(n, 4)
        raw = np.stack([x.min(1), y.min(1), x.max(1), y.max(1)], 1)
        new = np.stack([raw[:, 0].clip(0, W), raw[:, 1].clip(0, H), raw[:, 2].clip(0, W), raw[:, 3].clip(0, H)], 1)
        box1 = t[:, 1:5].T * mo.scale
        w1, h1 = box1[2] - box1[0], box1[3] - box1[1]
        w2, h2 = new[:, 2] - new[:, 0], new[:, 3] - new[:, 1]
        eps = 1e-16
        ar = np.maximum(w2 / (h2 + eps), h2 / (w2 + eps))
        area = w2 * h2 / (w1 * h1 + eps)
        keep = (w2 > 2) & (h2 > 2) & (area > 0.1) & (ar < 100)
        if check:
            assert box1.dtype == np.float32
            blas = (np.concatenate([p, np.ones((n * 4, 1))], 1) @ M.T)[:, :2].reshape(n, 8)
            raw_blas = np.stack([blas[:, 0::2].min(1), blas[:, 1::2].min(1), blas[:, 0::2].max(1), blas[:, 1::2].max(1)], 1)
            new_blas = np.stack([raw_blas[:, 0].clip(0, W), raw_blas[:, 1].clip(0, H), raw_blas[:, 2].clip(0, W), raw_blas[:, 3].clip(0, H)], 1)
            assert np.array_equal(new.astype(np.float32), new_blas.astype(np.float32)), "the plain fp64 sum and xy @ M.T round to different fp32 boxes"
            for v, thr in ((w2, 2.0), (h2, 2.0), (area, 0.1), (ar, 100.0)):
                assert (np.abs(v - thr) > 1e-9 * thr).all(), "a box_candidates comparison lies at its threshold"
        if stats is not None:
            stats["dropped"] += int((~keep).sum())
            if H != W:
                stats["cut_left"] += int((keep & (raw[:, 0] < 0)).sum())
                stats["cut_top"] += int((keep & (raw[:, 1] < 0)).sum())
                stats["cut_right"] += int((keep & (raw[:, 2] > W)).sum())
                stats["cut_bottom"] += int((keep & (raw[:, 3] > H)).sum())
        t = t[keep]
        t[:, 1:5] = new[keep]
    if len(t):
        t[:, 1:5] = xyxy2xywhn(t[:, 1:5], W, H)
        if item.flipud:
            t[:, 2] = 1 - t[:, 2]
        if item.fliplr:
            t[:, 1] = 1 - t[:, 1]
    return t


def batch_targets(items, labels, hw, H, W):
    """collate_fn over item_labels -> (nl, 6) fp32 [item in batch, cls, x, y, w, h]"""
    rows = []
    for b, it in enumerate(items):
        t = item_labels(it, labels, hw, H, W)
        rows.append(np.concatenate([np.full((len(t), 1), b, dtype=np.float32), t.astype(np.float32)], 1))
    return np.concatenate(rows, 0) if rows else np.zeros((0, 6), dtype=np.float32)
