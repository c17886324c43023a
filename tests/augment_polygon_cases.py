"""Shared inputs of the polygon-label tests of the train-mode dataset (tests/test_augment_polygons_cpu.py, tests/test_gpu_augment_polygons.py,
tests/golden/make_augment_polygons_golden.py): the twelve images of tests/augment_cases.py with polygon labels on most of them, the cases, and the NumPy statement of
the polygon label path as csrc/augment.hip computes it.  Not a test file.

The polygons: 3 to 40 vertices around the boxes of augment_cases.make_labels; one polygon of 1203 vertices (more than resample_segments' 1000 samples); one label file
with a plain box row among its polygon rows (the reference's parser reshapes its four numbers into a 2-point polygon); one polygon of a single vertex; one polygon whose
vertices are all (0, 0).  Images 4 and 10 keep box-only labels and image 7 has no labels, so that mosaics of every kind occur: all polygons, polygons mixed with boxes
(the box path), polygons with the label-less image (the polygon path).  The labels of a polygon image are the reference's own parse: segments2boxes of its polygons.

The statement (polygon_labels) is to the polygon path what model_labels of tests/golden/make_augment_golden.py is to the box path: fp32 where the reference's arrays
are fp32, fp64 where they are fp64, np.linspace and np.interp restated by their formulas, the transform as plain left-to-right sums in place of xy @ M.T.  The generator
asserts per polygon that both product forms keep the same points and round to the same fp32 box.
"""
from __future__ import annotations

import zlib

import numpy as np

import augment_cases as ac

IMG_SIZE, STRIDE, BATCH = ac.IMG_SIZE, ac.STRIDE, ac.BATCH
SAMPLES = 1000                    # resample_segments' n
BOX_ONLY = (3, 9)                 # images 000004 and 000010 keep box labels
MANY, MIXED_ROW, ZEROS, SINGLE = (2, 0), (4, 1), (7, 0), (11, 3)   # (image, row): 1203 vertices; written as a box row; all vertices (0, 0); one vertex
PATH_NONZERO, PATH_LACKS = 1, 2   # the bits of the per-mosaic word of y3_augment_polygons; the polygon path is taken when the word is PATH_NONZERO alone

# name -> hyp and the seeds / order of the epoch: the cases of augment_cases.py with seeds under which every situation of the generator's check_situations occurs
CASES = {
    "exact": dict(ac.CASES["exact"], seed=6),
    "low": dict(ac.CASES["low"], seed=6),
    "wild": dict(ac.CASES["wild"], seed=6),
    "single": dict(ac.CASES["single"], seed=6),
}


def _rng(what: str) -> np.random.RandomState:
    return np.random.RandomState(zlib.crc32(f"augment-polygons:{what}".encode()))


def _r6(a) -> np.ndarray:
    """what survives a label file: six decimals, then float32"""
    return np.array([float(f"{v:.6f}") for v in np.asarray(a, dtype=np.float64).reshape(-1)], dtype=np.float32).reshape(np.shape(a))


def segments2boxes(segments) -> np.ndarray:
    """(m, 4) float32 [x, y, w, h] of the polygons' extents, as the reference's parser derives the box columns (fp32 throughout)"""
    b = np.array([[p[:, 0].min(), p[:, 1].min(), p[:, 0].max(), p[:, 1].max()] for p in segments], dtype=np.float32).reshape(-1, 4)
    out = np.copy(b)
    out[:, 0], out[:, 1], out[:, 2], out[:, 3] = (b[:, 0] + b[:, 2]) / 2, (b[:, 1] + b[:, 3]) / 2, b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]
    return out


def make_polygons():
    """-> (labels, segments): per image (m, 5) float32 labels and a list of m (k, 2) float32 polygons (empty for the box-only and the label-less images)"""
    labels, segments = [], []
    for i, ((stem, _, _), lb) in enumerate(zip(ac.IMAGES, ac.make_labels())):
        if i in BOX_ONLY or not len(lb):
            labels.append(lb)
            segments.append([])
            continue
        rs, polys = _rng(stem), []
        for r, (_, xc, yc, bw, bh) in enumerate(lb.astype(np.float64)):
            if (i, r) == MIXED_ROW:
                polys.append(_r6([[xc, yc], [bw, bh]]))
                continue
            if (i, r) == ZEROS:
                polys.append(np.zeros((3, 2), dtype=np.float32))
                continue
            k = 1203 if (i, r) == MANY else (1 if (i, r) == SINGLE else int(rs.randint(3, 41)))
            ang = np.sort(rs.uniform(0, 2 * np.pi, k))
            rad = rs.uniform(0.45, 1.0, k)
            p = np.stack([xc + bw / 2 * rad * np.cos(ang), yc + bh / 2 * rad * np.sin(ang)], 1)
            polys.append(_r6(np.clip(p, 0.0, 1.0)))
        segments.append(polys)
        labels.append(np.concatenate([lb[:, :1], segments2boxes(polys)], 1).astype(np.float32))
    return labels, segments


def label_lines(i: int, labels, segments) -> list:
    """the rows of image i's label file: polygon rows `cls x1 y1 x2 y2 ...`, box rows `cls x y w h`"""
    if not len(segments[i]):
        return [" ".join([str(int(r[0]))] + [repr(float(v)) for v in r[1:]]) for r in labels[i]]
    return [" ".join([str(int(c))] + [repr(float(v)) for v in p.reshape(-1)]) for c, p in zip(labels[i][:, 0], segments[i])]


# ---- the statement ------------------------------------------------------------------------------------------------------------------------------------------------------
def xywhn2xyxy(x, w, h, padw, padh):
    y = np.empty_like(x)
    hw2, hh2 = x[..., 2] / 2, x[..., 3] / 2
    y[..., 0], y[..., 1] = w * (x[..., 0] - hw2) + padw, h * (x[..., 1] - hh2) + padh
    y[..., 2], y[..., 3] = w * (x[..., 0] + hw2) + padw, h * (x[..., 1] + hh2) + padh
    return y


def xyxy2xywhn_clip(x, s, eps=1e-3):
    x = x.copy()
    x[..., [0, 2]] = x[..., [0, 2]].clip(0, s - eps)
    x[..., [1, 3]] = x[..., [1, 3]].clip(0, s - eps)
    y = np.empty_like(x)
    y[..., 0], y[..., 1] = ((x[..., 0] + x[..., 2]) / 2) / s, ((x[..., 1] + x[..., 3]) / 2) / s
    y[..., 2], y[..., 3] = (x[..., 2] - x[..., 0]) / s, (x[..., 3] - x[..., 1]) / s
    return y


def canvas_polygon(p, w, h, padw, padh, canvas):
    """xyn2xy and load_mosaic's clip, fp32: (k, 2) float32 -> (k, 2) float32"""
    assert p.dtype == np.float32
    y = np.copy(p)
    y[:, 0] = w * p[:, 0] + padw
    y[:, 1] = h * p[:, 1] + padh
    assert y.dtype == np.float32
    return np.clip(y, 0, canvas)


def resample(p):
    """resample_segments for one polygon: (k, 2) float32 -> (1000, 2) float64.  np.linspace(0, k, 1000) is i (k / 999) with the last element k; np.interp over
    xp = arange(k + 1) of the closed polygon is (b - a) (t - q) + a with q = floor(t), a itself where t == q, and the closing vertex at t == k."""
    k = len(p)
    closed = np.concatenate([p, p[:1]], 0).astype(np.float64)
    t = np.arange(SAMPLES, dtype=np.float64) * (float(k) / (SAMPLES - 1))
    t[-1] = float(k)
    q = np.minimum(t.astype(np.int64), k)
    a, b = closed[q], closed[np.minimum(q + 1, k)]
    return np.where(((q == k) | (t == q))[:, None], a, (b - a) * (t - q)[:, None] + a)


def warp_points(p, M):
    """the 1000 samples of one polygon on the canvas (float32) through M as plain left-to-right sums -> X, Y float64"""
    xy = resample(p)
    return xy[:, 0] * M[0, 0] + xy[:, 1] * M[0, 1] + M[0, 2], xy[:, 0] * M[1, 0] + xy[:, 1] * M[1, 1] + M[1, 2]


def polygon_box(p, M, s):
    """one polygon on the canvas (float32) through M -> (box (4,) float64, taken): segment2box of the plain-sum transform of its 1000 samples"""
    X, Y = warp_points(p, M)
    inside = (X >= 0) & (Y >= 0) & (X <= s) & (Y <= s)
    X, Y = X[inside], Y[inside]
    if not (X != 0).any():   # segment2box's any(x): no point kept, or every kept x zero
        return np.zeros(4), False
    return np.array([X.min(), Y.min(), X.max(), Y.max()]), True


def corner_boxes(t, M, s):
    """the box path's `new`: the four corners of t (n, 4) float32 through M as plain sums, min / max, clipped to [0, s] -> (n, 4) float64"""
    n = len(t)
    p = t[:, [0, 1, 2, 3, 0, 3, 2, 1]].reshape(n * 4, 2).astype(np.float64)
    x = (p[:, 0] * M[0, 0] + p[:, 1] * M[0, 1] + M[0, 2]).reshape(n, 4)
    y = (p[:, 0] * M[1, 0] + p[:, 1] * M[1, 1] + M[1, 2]).reshape(n, 4)
    return np.stack([x.min(1), y.min(1), x.max(1), y.max(1)], 1).clip(0, s)


def candidates(t, new, scale, area_thr):
    """box_candidates(box1 = t.T * scale (fp32), box2 = new.T (fp64)) -> (keep, (w2, h2, area, ar))"""
    box1 = t.T * scale
    assert box1.dtype == np.float32
    w1, h1 = box1[2] - box1[0], box1[3] - box1[1]
    w2, h2 = new[:, 2] - new[:, 0], new[:, 3] - new[:, 1]
    eps = 1e-16
    ar = np.maximum(w2 / (h2 + eps), h2 / (w2 + eps))
    area = w2 * h2 / (w1 * h1 + eps)
    return (w2 > 2) & (h2 > 2) & (area > area_thr) & (ar < 100), (w2, h2, area, ar)


def polygon_labels(item, labels, segments, hw, s):
    """The label path of one drawn item (yolov3_amd.augment.Item) over a set with polygons -> dict(targets (nl, 5) float32 [cls, x, y, w, h]; per mosaic: `words` the
    path word, `boxes` (n, 4) float64 and `inside` (n,) the polygon boxes of its label rows in tile order (zeros for a row without a polygon; None for the letterbox
    branch, which hands no segments on), `rows` what the rows were before the filter (n, 5) float32, `new` and `keep` what the filter saw, `polys` the polygons on the canvas (None for a row without one))."""
    out = dict(targets=None, words=[], boxes=[], inside=[], rows=[], new=[], keep=[], polys=[])
    kept = []
    for mo in item.mosaics:
        rows, polys = [], []
        for j, (padw, padh) in zip(mo.indices, mo.pad):
            lb = labels[j].copy()
            if lb.size:
                lb[:, 1:] = xywhn2xyxy(lb[:, 1:], hw[j][1], hw[j][0], padw, padh)
                if item.mosaic:
                    polys += [canvas_polygon(p, hw[j][1], hw[j][0], padw, padh, mo.canvas) for p in segments[j]] if len(segments[j]) else [None] * len(lb)
            rows.append(lb)
        t = np.concatenate(rows, 0)
        n = len(t)
        word, boxes, inside = 0, None, None
        if item.mosaic:
            np.clip(t[:, 1:], 0, mo.canvas, out=t[:, 1:])
            word = (PATH_NONZERO if any(p is not None and p.any() for p in polys) else 0) | (PATH_LACKS if any(p is None for p in polys) else 0)
            got = [polygon_box(p, mo.M, s) if p is not None else (np.zeros(4), False) for p in polys]
            boxes, inside = np.array([g[0] for g in got], dtype=np.float64).reshape(n, 4), np.array([g[1] for g in got], dtype=bool)
        new, keep = np.zeros((n, 4)), np.zeros(n, dtype=bool)
        if n:
            poly = word == PATH_NONZERO
            new = boxes if poly else corner_boxes(t[:, 1:5], mo.M, s)
            keep, _ = candidates(t[:, 1:5], new, mo.scale, 0.01 if poly else 0.10)
        for key, v in (("words", word), ("boxes", boxes), ("inside", inside), ("rows", t.copy()), ("new", new), ("keep", keep), ("polys", polys)):
            out[key].append(v)
        t = t[keep]
        t[:, 1:5] = new[keep]
        kept.append(t)
    t = np.concatenate(kept, 0)
    if len(t):
        t[:, 1:5] = xyxy2xywhn_clip(t[:, 1:5], s)
        if item.flipud:
            t[:, 2] = 1 - t[:, 2]
        if item.fliplr:
            t[:, 1] = 1 - t[:, 1]
    assert t.dtype == np.float32
    out["targets"] = t
    return out


def batch_statement(items, labels, segments, hw, s):
    """a batch as the device lays it out -> dict(targets (nl, 6) float32, boxes (upper, 4) float64, inside (upper,) int32, written (upper,) bool: the positions the
    polygon launch writes (the rows of mosaic items), words (count, 2) int32)"""
    targets, boxes, inside, written, words = [], [], [], [], np.zeros((len(items), 2), dtype=np.int32)
    for b, it in enumerate(items):
        st = polygon_labels(it, labels, segments, hw, s)
        targets.append(np.concatenate([np.full((len(st["targets"]), 1), b, dtype=np.float32), st["targets"]], 1))
        for m, (word, bx, ins, rows) in enumerate(zip(st["words"], st["boxes"], st["inside"], st["rows"])):
            words[b, m] = word
            n = len(rows)
            boxes.append(np.zeros((n, 4)) if bx is None else bx)
            inside.append(np.zeros(n, dtype=np.int32) if ins is None else ins.astype(np.int32))
            written.append(np.full(n, bx is not None))
    return dict(targets=np.concatenate(targets, 0).astype(np.float32).reshape(-1, 6), boxes=np.concatenate(boxes, 0).reshape(-1, 4),
                inside=np.concatenate(inside, 0).astype(np.int32), written=np.concatenate(written, 0).astype(bool), words=words)


def zero_polygon_set():
    """The one situation the reference's parser cannot produce (there the box clips to zero with its polygon): every polygon of a mosaic clips to all zeros while the
    label boxes do not, so the mosaic falls back to the box path.  Images 0 .. 3 of the set, every label row with a polygon far up and left of its image (vertices
    (-10, -10): beyond the canvas origin wherever the tile is pasted) and its box left as augment_cases.make_labels has it -> (images, labels, segments, hw).
    Expectations come from the statement alone."""
    images, labels = ac.make_images()[:4], ac.make_labels()[:4]
    return images, labels, [[np.full((3 + r, 2), -10.0, dtype=np.float32) for r in range(len(lb))] for lb in labels], ac.hw()[:4]
