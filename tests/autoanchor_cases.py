"""Shared inputs of the autoanchor tests (tests/test_autoanchor_cpu.py, tests/test_gpu_autoanchor.py, tests/golden/make_autoanchor_golden.py): the seeded
fake datasets, and a plain NumPy restatement of the whole procedure (reference utils/autoanchor.py with scipy.cluster.vq.kmeans behind it) in this project's own
words -- fp32 ratio metric with fp64 sums, a Lloyd loop with scipy's stopping rule and empty-code drop, the genetic loop.  Not a test file."""
from __future__ import annotations

import random
import types

import numpy as np

# name -> images, mean labels per image (None: 3 each), n anchors, generations, the seed of the dataset (B runs on A's dataset); E is built by hand below.
# The golden's generator searches the seed of the RANDOM STREAMS (0..31) per case; a dataset seed is the first for which that search succeeds.
CASES = {
    "A": dict(n_img=97, lam=3.2, n=9, gen=300, dseed=0),
    "B": dict(n_img=97, lam=3.2, n=6, gen=300, dseed=0),
    "C": dict(n_img=1300, lam=3.3, n=9, gen=50, dseed=0),
    "D": dict(n_img=3, lam=None, n=9, gen=50, dseed=0),
    "E": dict(n_img=8, lam=None, n=9, gen=20, dseed=0),
}
IMG_SIZE, THR = 640, 4.0
RESTARTS, KM_THRESH = 30, 1e-5
ANCHORS = {   # (pixel anchors, strides) of the two model families
    "yolov3": ([[10, 13, 16, 30, 33, 23], [30, 61, 62, 45, 59, 119], [116, 90, 156, 198, 373, 326]], [8.0, 16.0, 32.0]),
    "yolov3-tiny": ([[10, 14, 23, 27, 37, 58], [81, 82, 135, 169, 344, 319]], [16.0, 32.0]),
}


def make_dataset(case: str, dseed: int | None = None):
    """.shapes (n_img, 2) int64 and .labels (list of (m, 5) float32 [cls, x, y, w, h] normalised), from a generator of its own (the global streams stay untouched)"""
    c = CASES[case]
    rs = np.random.RandomState(7919 * ((c["dseed"] if dseed is None else dseed) + 1) + (0 if case in "AB" else ord(case)))
    n_img = c["n_img"]
    if case == "E":   # 40 labels of 5 distinct sizes on square images: k-means for 9 codes loses codes
        sizes = np.array([[0.05, 0.08], [0.12, 0.1], [0.3, 0.22], [0.5, 0.61], [0.81, 0.7]], dtype=np.float32)
        shapes = np.full((n_img, 2), 640, dtype=np.int64)
        labels = [np.concatenate([np.zeros((5, 1), np.float32), np.full((5, 2), 0.5, np.float32), sizes], 1) for _ in range(n_img)]
        return types.SimpleNamespace(shapes=shapes, labels=labels)
    shapes = rs.randint(320, 1281, size=(n_img, 2)).astype(np.int64)
    counts = np.full(n_img, 3) if c["lam"] is None else rs.poisson(c["lam"], n_img)
    labels = []
    for m in counts:
        wh = np.exp(rs.normal(np.log(0.12), 0.95, size=(m, 2))).clip(0.004, 0.95)
        lb = np.concatenate([rs.randint(0, 80, (m, 1)).astype(np.float64), rs.uniform(0.1, 0.9, (m, 2)), wh], 1)
        labels.append(lb.astype(np.float32))
    return types.SimpleNamespace(shapes=shapes, labels=labels)


def dataset_checksum(ds) -> float:
    return float(ds.shapes.astype(np.float64).sum() + sum(float(l.astype(np.float64).sum()) for l in ds.labels))


def seed_all(seed: int):
    np.random.seed(seed)
    random.seed(seed)


def label_wh(ds, img_size, scale=None):
    shapes = img_size * ds.shapes / ds.shapes.max(1, keepdims=True)
    if scale is not None:
        shapes = shapes * scale
    return np.concatenate([l[:, 3:5] * s for s, l in zip(shapes, ds.labels)])


# ---- the ratio metric -------------------------------------------------------------------------------------------------------------
def ratio_metric(wh, k):
    """x (N, n) and best (N,) in fp32: every label size against every anchor, the worse of the two side ratios, each ratio folded below 1"""
    wh, k = np.asarray(wh, dtype=np.float32), np.asarray(k).astype(np.float32)
    with np.errstate(divide="ignore"):
        r = wh[:, None, :] / k[None]
        x = np.minimum(r, np.float32(1.0) / r).min(2)
    return x, x.max(1)


def metrics(wh, k, thr=THR) -> dict:
    x, best = ratio_metric(wh, k)
    t = np.float32(1.0 / thr)
    N, n = x.shape
    n_best, n_x = int((best > t).sum()), int((x > t).sum())
    return {
        "N": N, "n": n, "n_best_past": n_best, "n_x_past": n_x,
        "bpr": np.float32(n_best) / np.float32(N), "aat": np.float32(n_x) / np.float32(N),
        "fitness": float(best[best > t].astype(np.float64).sum()) / N,
        "x_mean": float(x.astype(np.float64).sum()) / (N * n), "best_mean": float(best.astype(np.float64).sum()) / N,
        "past_thr_mean": float(x[x > t].astype(np.float64).sum()) / n_x if n_x else float("nan"),
    }


def fitness(wh, k, thr=THR) -> float:
    _, best = ratio_metric(wh, k)
    return float(best[best > np.float32(1.0 / thr)].astype(np.float64).sum()) / len(best)


# ---- k-means ------------------------------------------------------------------------------------------------------------------------
def lloyd(obs, idx, trace=None):
    """one restart from obs[idx] in fp64 -> (codebook of the codes that kept members, mean distance before the last update, iterations).  trace (a dict)
    collects how close the run came to a rounding edge: the |change of the mean distance| of every iteration and the smallest relative gap between a point's
    nearest and second nearest code."""
    obs = np.asarray(obs, dtype=np.float64)
    book = obs[np.asarray(idx)].copy()
    prev, it = np.inf, 0
    while True:
        d2 = ((obs[:, None, :] - book[None]) ** 2).sum(-1)
        code = d2.argmin(1)   # the first smallest: ties to the lowest index
        dist = np.sqrt(d2[np.arange(len(obs)), code])
        d = dist.sum() / len(obs)
        it += 1
        if trace is not None and book.shape[0] > 1:
            s = np.sqrt(np.sort(d2, 1)[:, :2])
            trace.setdefault("gap", []).append(float(((s[:, 1] - s[:, 0]) / np.maximum(s[:, 1], 1e-300)).min()))
        new = []
        for j in range(book.shape[0]):
            m = code == j
            if m.any():
                new.append(obs[m].sum(0) / m.sum())
        book = np.array(new)
        diff = abs(prev - d)
        if trace is not None and np.isfinite(diff):
            trace.setdefault("delta", []).append(float(diff))
        prev = d
        if diff <= KM_THRESH:
            return book, d, it


def kmeans(obs, index_sets, trace=None):
    """the restarts of scipy.cluster.vq.kmeans(obs, n, iter=len(index_sets)): the first restart with the smallest mean distance wins"""
    best, iters = None, []
    for idx in index_sets:
        book, d, it = lloyd(obs, idx, trace)
        iters.append(it)
        if best is None or d < best[1]:
            best = (book, d)
    return best[0], best[1], np.array(iters)


# ---- the genetic loop -----------------------------------------------------------------------------------------------------------------
def draw_mutations(gen, shape):
    """the reference's draw (utils/autoanchor.py:153-155) from the global NumPy and Python streams"""
    npr, mp, s = np.random, 0.9, 0.1
    out = np.ones((gen, *shape))
    for g in range(gen):
        v = np.ones(shape)
        while (v == 1).all():
            v = ((npr.random(shape) < mp) * random.random() * npr.randn(*shape) * s + 1).clip(0.3, 3.0)
        out[g] = v
    return out


def evolve(wh, k0, v, thr=THR):
    """-> (anchors, accepted mask, fitness of every candidate, fitness of the start): a candidate replaces the anchors when it is strictly fitter"""
    k = np.asarray(k0, dtype=np.float64).copy()
    f0 = f = fitness(wh, k, thr)
    acc, fgs = np.zeros(len(v), dtype=np.int32), np.zeros(len(v))
    for g in range(len(v)):
        kg = (k * v[g]).clip(min=2.0)
        fgs[g] = fg = fitness(wh, kg, thr)
        if fg > f:
            f, k, acc[g] = fg, kg, 1
    return k, acc, fgs, f0


def by_area(k):
    return k[np.argsort(k.prod(1))]


def kmean_anchors(ds, n=9, img_size=IMG_SIZE, thr=THR, gen=1000, init=None, mutations=None, record=None):
    """the whole of the reference's kmean_anchors, consuming the global random streams as it does -> float32 (n, 2) sorted by area"""
    record = {} if record is None else record
    wh0 = label_wh(ds, img_size)
    wh = wh0[(wh0 >= 2.0).any(1)].astype(np.float32)
    if init is not None:
        k = np.asarray(init, dtype=np.float64)
    else:
        k = None
        if n <= len(wh):
            s = wh.std(0)
            index_sets = [np.random.choice(wh.shape[0], size=n, replace=False) for _ in range(RESTARTS)]
            book, d, iters = kmeans(wh / s, index_sets)
            record.update(index_sets=np.array(index_sets), book=book, distortion=d, kmeans_iters=iters)
            if len(book) == n:
                k = book * s.astype(np.float64)
        if k is None:
            k = np.sort(np.random.rand(n * 2)).reshape(n, 2) * img_size
            record["fallback"] = True
    k = by_area(k)
    v = draw_mutations(gen, k.shape) if mutations is None else np.asarray(mutations)
    record.update(k0=k.copy(), v=v)
    k, acc, fgs, f0 = evolve(wh, k, v, thr)
    record.update(accepted=acc, fitness=fgs)
    return by_area(k).astype(np.float32)


def check_anchors(ds, anchors, strides, thr=THR, imgsz=IMG_SIZE, record=None):
    """the reference's check_anchors on plain arrays: anchors (nl, na, 2) in grid units -> the anchors after the call (grid units, float32)"""
    record = {} if record is None else record
    anchors = np.asarray(anchors, dtype=np.float32)
    stride = np.asarray(strides, dtype=np.float32).reshape(-1, 1, 1)
    scale = np.random.uniform(0.9, 1.1, size=(ds.shapes.shape[0], 1))
    wh = label_wh(ds, imgsz, scale).astype(np.float32)
    bpr = metrics(wh, (anchors * stride).reshape(-1, 2), thr)["bpr"]
    record.update(wh=wh, bpr=bpr)
    if bpr > 0.98:
        return anchors
    new = kmean_anchors(ds, n=anchors.size // 2, img_size=imgsz, thr=thr, gen=1000)
    record["new_bpr"] = new_bpr = metrics(wh, new, thr)["bpr"]
    if not new_bpr > bpr:
        return anchors
    a = new.reshape(anchors.shape)
    area = a.prod(-1).mean(-1)
    if (area[-1] - area[0]) and np.sign(area[-1] - area[0]) != np.sign(stride[-1, 0, 0] - stride[0, 0, 0]):
        a = a[::-1]
    return (a / stride).astype(np.float32)
