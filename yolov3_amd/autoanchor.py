"""Autoanchor on the device (reference utils/autoanchor.py): check_anchors, kmean_anchors, check_anchor_order.

What the reference's train.py runs on the host before the first batch -- the ratio metric of every label against every anchor, scipy's k-means and the
1000-generation genetic loop -- runs here through csrc/autoanchor.hip (y3_anchor_metrics / y3_kmeans_step / y3_anchor_evolve).  The host keeps what is not
arithmetic over the labels: building the (N, 2) table of label sizes with NumPy exactly as the reference builds it, and drawing the random numbers in the
reference's order from the global NumPy / Python generators, so a seeded run consumes both streams as the reference does.

Differences from the reference, all deliberate:
  * errors propagate (the reference's @TryExcept swallows them);
  * a dataset given as a *.yaml path raises NotImplementedError (the dataloader is out of scope);
  * `verbose` logs the final summary line and the number of accepted generations, not one line per accepted generation: the loop never returns to the host;
  * k-means runs its 30 restarts side by side in fp64 (scipy: one after the other in fp32); the initial points of every restart are drawn first, which leaves
    the NumPy stream where scipy leaves it;
  * sums are fp64 in a fixed order: results are run-to-run bit-identical.
"""
from __future__ import annotations

import logging
import random

import numpy as np
import torch

from . import ops
from .yolo import check_anchor_order  # noqa: F401  (re-exported: reference utils/autoanchor.py:16-23)

LOGGER = logging.getLogger("yolov3_amd")
PREFIX = "AutoAnchor: "
KMEANS_RESTARTS = 30     # kmeans(wh / s, n, iter=30)
KMEANS_THRESH = 1e-5     # scipy.cluster.vq.kmeans(thresh=1e-5)


def _device_k(k, device) -> torch.Tensor:
    if isinstance(k, torch.Tensor):
        return k.detach().to(device=device, dtype=torch.float64).reshape(-1, 2).contiguous()
    return torch.from_numpy(np.ascontiguousarray(np.asarray(k, dtype=np.float64).reshape(-1, 2))).to(device)


def anchor_metrics(wh: torch.Tensor, k, thr: float = 4.0) -> dict:
    """Every figure check_anchors.metric, anchor_fitness and print_results form from the ratio metric of the (N, 2) fp32 label sizes `wh` (on the GPU) against the
    anchors `k` ((n, 2), any array; rounded to fp32 as the reference's torch.tensor(k, dtype=torch.float32)), thr = hyp['anchor_t'].  One device pass, one read."""
    ops.require_gpu(wh, "anchor_metrics")
    kd = _device_k(k, wh.device)
    N, n = int(wh.shape[0]), int(kd.shape[0])
    t = ops.anchor_metrics(wh, kd, np.float32(1.0 / thr)).cpu().tolist()
    n_best, n_x = int(t[1]), int(t[2])
    return {
        "N": N, "n": n, "n_best_past": n_best, "n_x_past": n_x,
        "bpr": np.float32(n_best) / np.float32(N),            # (best > 1 / thr).float().mean()
        "aat": np.float32(n_x) / np.float32(N),                # (x > 1 / thr).float().sum(1).mean()
        "fitness": t[0] / N,                                   # (best * (best > thr).float()).mean()
        "x_mean": t[3] / (N * n), "best_mean": t[4] / N,        # print_results: metric_all
        "past_thr_mean": t[5] / n_x if n_x else float("nan"),  # x[x > thr].mean()
    }


def _label_wh(dataset, img_size, scale=None) -> np.ndarray:
    shapes = img_size * dataset.shapes / dataset.shapes.max(1, keepdims=True)
    if scale is not None:
        shapes = shapes * scale
    return np.concatenate([label[:, 3:5] * shape for shape, label in zip(shapes, dataset.labels)])


def _kmeans_device(obs: np.ndarray, index_sets, device, max_iter: int = 10000):
    """(Not public: kmean_anchors' k-means stage, named so that the tests can drive it from recorded initial points.)  Lloyd's algorithm as scipy.cluster.vq.kmeans runs it, for all restarts at once on the device: restart r starts from obs[index_sets[r]] and stops when the
    mean distance moved by at most 1e-5; a code without members is dropped for the rest of its restart.
    -> (best codebook (live rows only, fp64), its mean distance, iterations of every restart)"""
    idx = np.asarray(index_sets, dtype=np.int64)
    R, n = idx.shape
    if not 1 <= R <= 64:
        raise ValueError(f"kmeans: {R} restarts unsupported (1 .. 64)")
    obs = np.ascontiguousarray(obs, dtype=np.float32)
    pts = torch.from_numpy(obs).to(device)
    codes = torch.from_numpy(obs[idx].astype(np.float64)).to(device).contiguous()
    live = torch.ones(R, n, dtype=torch.int32, device=device)
    dist = torch.zeros(R, dtype=torch.float64, device=device)
    prev = np.full(R, np.inf)
    final = np.full(R, np.inf)
    iters = np.zeros(R, dtype=np.int64)
    frozen = 0
    full = (1 << R) - 1
    for _ in range(max_iter):
        if frozen == full:
            break
        ops.kmeans_step(pts, codes, live, frozen, dist)
        d = dist.cpu().numpy()   # the one device -> host copy of the iteration
        for r in range(R):
            if (frozen >> r) & 1:
                continue
            iters[r] += 1
            if abs(prev[r] - d[r]) <= KMEANS_THRESH:
                frozen |= 1 << r
                final[r] = d[r]
            prev[r] = d[r]
    if frozen != full:
        raise RuntimeError(f"kmeans: no convergence within {max_iter} iterations")
    best = int(np.argmin(final))   # scipy keeps the first restart with the smallest distance (dist < best_dist)
    book = codes[best].cpu().numpy()[live[best].cpu().numpy().astype(bool)]
    return book, float(final[best]), iters


def kmean_anchors(dataset="./data/coco128.yaml", n=9, img_size=640, thr=4.0, gen=1000, verbose=True, *, init=None, mutations=None, device=None, record=None):
    """Create k-means evolved anchors from a training dataset (reference utils/autoanchor.py:67-164) -> np.float32 (n, 2), sorted by area.

    dataset: an object with .shapes (n_img, 2) and .labels (list of (m, 5) arrays).  init: (n, 2) anchors that replace the k-means result; mutations:
    (gen, n, 2) factors that replace the drawn ones -- both for tests that drive a stage from recorded data.  record: a dict that receives the intermediate
    results (k0, v, accepted, fitness, kmeans_iters)."""
    if isinstance(dataset, str):
        raise NotImplementedError("kmean_anchors: a *.yaml dataset path needs the reference's dataloader, which is out of scope; pass a dataset with .shapes and .labels")
    if not torch.cuda.is_available() and device is None:
        raise RuntimeError("kmean_anchors: no CPU / PyTorch fallback; the yolov3_amd hot path runs only on an MI355X (HIP) device.")
    device = torch.device(device if device is not None else "cuda")
    ops.require_gpu(torch.empty(0, device=device), "kmean_anchors")
    npr = np.random
    record = {} if record is None else record

    wh0 = _label_wh(dataset, img_size)
    i = (wh0 < 3.0).any(1).sum()
    if i:
        LOGGER.warning(f"{PREFIX}Extremely small objects found: {i} of {len(wh0)} labels are <3 pixels in size")
    wh = wh0[(wh0 >= 2.0).any(1)].astype(np.float32)

    if init is not None:
        k = np.asarray(init, dtype=np.float64).reshape(n, 2)
    else:
        k = None
        LOGGER.info(f"{PREFIX}Running kmeans for {n} anchors on {len(wh)} points...")
        if n <= len(wh):
            s = wh.std(0)
            index_sets = [npr.choice(wh.shape[0], size=int(n), replace=False) for _ in range(KMEANS_RESTARTS)]
            book, _, iters = _kmeans_device(wh / s, index_sets, device)
            record["kmeans_iters"] = iters
            if len(book) == n:
                k = book * s.astype(np.float64)
        if k is None:
            LOGGER.warning(f"{PREFIX}switching strategies from kmeans to random init")
            k = np.sort(npr.rand(n * 2)).reshape(n, 2) * img_size
    k = k[np.argsort(k.prod(1))]
    record["k0"] = k.copy()

    if mutations is not None:
        v = np.asarray(mutations, dtype=np.float64).reshape(-1, n, 2)
    else:
        sh, mp, s = k.shape, 0.9, 0.1
        v = np.ones((gen, *sh))
        for g in range(gen):
            while (v[g] == 1).all():   # mutate until a change occurs (the reference's expression, verbatim)
                v[g] = ((npr.random(sh) < mp) * random.random() * npr.randn(*sh) * s + 1).clip(0.3, 3.0)
    record["v"] = v

    whd = torch.from_numpy(wh).to(device)
    kd = torch.from_numpy(np.ascontiguousarray(k)).to(device)
    f, accepted = ops.anchor_evolve(whd, kd, torch.from_numpy(np.ascontiguousarray(v)).to(device), np.float32(1.0 / thr))
    k = kd.cpu().numpy()
    record["accepted"], record["fitness"] = accepted.cpu().numpy(), float(f.cpu())
    k = k[np.argsort(k.prod(1))]
    if verbose:
        r = anchor_metrics(torch.from_numpy(wh0.astype(np.float32)).to(device), k, thr)
        LOGGER.info(f"{PREFIX}Evolved anchors with Genetic Algorithm: fitness = {record['fitness']:.4f}, {int(record['accepted'].sum())} of {len(v)} generations accepted")
        LOGGER.info(f"{PREFIX}thr={1 / thr:.2f}: {r['n_best_past'] / r['N']:.4f} best possible recall, {r['n_x_past'] / r['N']:.2f} anchors past thr\n"
                    f"{PREFIX}n={n}, img_size={img_size}, metric_all={r['x_mean']:.3f}/{r['best_mean']:.3f}-mean/best, past_thr={r['past_thr_mean']:.3f}-mean: "
                    + ", ".join(f"{round(a[0])},{round(a[1])}" for a in k))
    return k.astype(np.float32)


def check_anchors(dataset, model, thr=4.0, imgsz=640):
    """Evaluate anchor fit to a dataset and recompute anchors with k-means if best possible recall is too low (reference utils/autoanchor.py:27-64).
    New anchors are written into m.anchors IN PLACE: ComputeLoss and the engine's plan cache watch the buffer's version counter."""
    m = model.module.model[-1] if hasattr(model, "module") else model.model[-1]   # Detect()
    ops.require_gpu(m.anchors, "check_anchors")
    device = m.anchors.device
    scale = np.random.uniform(0.9, 1.1, size=(dataset.shapes.shape[0], 1))   # augment scale
    wh = torch.tensor(_label_wh(dataset, imgsz, scale)).float().to(device)

    stride = m.stride.to(device).view(-1, 1, 1)
    anchors = m.anchors.clone() * stride
    r = anchor_metrics(wh, anchors.view(-1, 2), thr)
    bpr, aat = r["bpr"], r["aat"]
    s = f"\n{PREFIX}{aat:.2f} anchors/target, {bpr:.3f} Best Possible Recall (BPR). "
    if bpr > 0.98:
        LOGGER.info(f"{s}Current anchors are a good fit to dataset")
        return
    LOGGER.info(f"{s}Anchors are a poor fit to dataset, attempting to improve...")
    na = m.anchors.numel() // 2
    anchors = kmean_anchors(dataset, n=na, img_size=imgsz, thr=thr, gen=1000, verbose=False, device=device)
    new_bpr = anchor_metrics(wh, anchors, thr)["bpr"]
    if new_bpr > bpr:
        anchors = torch.tensor(anchors, device=device).type_as(m.anchors)
        m.anchors[:] = anchors.clone().view_as(m.anchors)
        check_anchor_order(m)   # must be in pixel-space (not grid-space)
        m.anchors /= stride
        LOGGER.info(f"{PREFIX}Done (optional: update model *.yaml to use these anchors in the future)")
    else:
        LOGGER.info(f"{PREFIX}Done (original anchors better than new anchors, proceeding with original anchors)")
