"""Shared inputs of the class / image weight tests (tests/test_label_weights_cpu.py, tests/test_gpu_label_weights.py, tests/golden/make_label_weights_golden.py):
the seeded label lists, each the smallest shape at which one thing can go wrong, and the per-class mAPs of the epoch prologue.  Not a test file.

  A  257 images, nc 80, 0 .. 40 labels each, the first and the last image empty, every seventh id stored as c + 0.7: segment ends, truncation, a label count
     that is no multiple of 64 or 256
  B  64 images, nc 1: a single class
  C  1031 images, nc 365, 40 classes used: empty bins replaced by 1, nc above a wave and above a block
  D  33 images, nc 80, image 7 with 5000 labels, ten images empty: one long segment
  E  16 images, nc 80, all empty: zero total
  F  20 000 images, about 150 000 labels, nc 80: many blocks, ten scan chunks with carries
"""
from __future__ import annotations

import zlib
from itertools import accumulate

import numpy as np

CASES = {
    "A": dict(n_img=257, nc=80),
    "B": dict(n_img=64, nc=1),
    "C": dict(n_img=1031, nc=365),
    "D": dict(n_img=33, nc=80),
    "E": dict(n_img=16, nc=80),
    "F": dict(n_img=20_000, nc=80),
}
MARGIN = 1e-9   # every draw u * total of a golden seed lies at least MARGIN * total away from every cumulative boundary


def _rng(case: str) -> np.random.RandomState:
    return np.random.RandomState(zlib.crc32(f"label_weights:{case}".encode()))   # seeded from the case's name; the global streams stay untouched


def make_labels(case: str) -> list:
    """dataset.labels of the case: a list of (m, 5) float32 arrays [class, x, y, w, h]"""
    c = CASES[case]
    rs, n_img, nc = _rng(case), c["n_img"], c["nc"]
    if case == "A":
        counts = rs.randint(0, 41, n_img)
        counts[0] = counts[-1] = 0
    elif case == "B":
        counts = rs.randint(0, 6, n_img)
    elif case == "C":
        counts = rs.poisson(4.0, n_img)
    elif case == "D":
        counts = rs.randint(1, 9, n_img)
        counts[rs.choice(np.setdiff1d(np.arange(n_img), [7]), 10, replace=False)] = 0
        counts[7] = 5000
    elif case == "E":
        counts = np.zeros(n_img, dtype=np.int64)
    else:
        counts = rs.poisson(7.5, n_img)
    used = np.sort(rs.choice(nc, 40, replace=False)) if case == "C" else np.arange(nc)
    labels = []
    for m in counts:
        ids = used[rs.randint(0, len(used), m)].astype(np.float64)
        if case == "A":
            ids[::7] += 0.7
        labels.append(np.concatenate([ids[:, None], rs.uniform(0.05, 0.95, (m, 4))], 1).astype(np.float32))
    return labels


def make_maps(case: str) -> np.ndarray:
    """per-class mAP of the previous epoch, what run_batches returns as `maps`: float64 (nc,) in [0, 1)"""
    return np.random.RandomState(zlib.crc32(f"label_weights:maps:{case}".encode())).uniform(0.0, 1.0, CASES[case]["nc"])


def checksum(labels) -> float:
    return float(len(labels) + sum(float(l.astype(np.float64).sum()) + 3.0 * len(l) for l in labels))


def class_ids(labels) -> np.ndarray:
    return np.concatenate(labels, 0)[:, 0].astype(int)


def boundary_margin(iw: np.ndarray, us) -> float:
    """the smallest |u * total - cumulative boundary| / total over the draws `us`, for the cumulative weights random.choices forms (itertools.accumulate)"""
    cum = np.array(list(accumulate(iw.tolist())))
    total = cum[-1]
    x = np.asarray(us) * total
    pos = np.searchsorted(cum, x)
    lo, hi = cum[np.clip(pos - 1, 0, len(cum) - 1)], cum[np.clip(pos, 0, len(cum) - 1)]
    return float(np.minimum(np.abs(x - lo), np.abs(x - hi)).min() / total)
