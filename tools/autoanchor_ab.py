"""A/B of autoanchor at COCO scale on one MI355X, in interleaved rounds: the device path (csrc/autoanchor.hip through yolov3_amd/autoanchor.py) against the host
restatement of tests/autoanchor_cases.py (NumPy: the reference's torch-CPU arithmetic in fp32 with fp64 sums; shared with the tests, as tools/val_stats_ab.py
shares its host form, so that what is timed is what is tested) on a synthetic table of label sizes.  scipy is not used.

  fitness    one anchor_fitness evaluation (the reference runs 1000 of them in its genetic loop)          device: y3_anchor_metrics incl. the read-back
  evolve     --gen generations of the genetic loop                                                        device: y3_anchor_evolve, one read at the end
  kmeans     --restarts k-means restarts from the same initial points, --km-iters Lloyd iterations each   device: y3_kmeans_step, one read per iteration
             (host: an fp64 NumPy Lloyd loop with bincount sums, restart after restart, as scipy runs them)

Every round times each arm once, the arms alternate within a round; medians over the rounds and the ratio host / device are printed.  No speed-up is promised:
the report records what was measured.

    python tools/autoanchor_ab.py [--labels 860000] [--rounds 3] [--gen 20] [--restarts 30] [--km-iters 3] [--out profiles/autoanchor_ab.txt]
"""
import argparse
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import autoanchor_cases as ac  # noqa: E402
from yolov3_amd import anchor_metrics, ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--labels", type=int, default=860_000)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--gen", type=int, default=20)
ap.add_argument("--restarts", type=int, default=30)
ap.add_argument("--km-iters", type=int, default=3)
ap.add_argument("--out", default=str(ROOT / "profiles" / "autoanchor_ab.txt"), help="the report is also written to this file ('' for none)")
args = ap.parse_args()
assert torch.cuda.is_available(), "autoanchor_ab.py measures on an MI355X; there is nothing to measure without one"
dev = torch.device("cuda:0")

rs = np.random.RandomState(0)
wh = (np.exp(rs.normal(np.log(0.1), 0.9, size=(args.labels, 2))).clip(0.004, 0.95) * 640).astype(np.float32)
k0 = np.array(ac.ANCHORS["yolov3"][0], dtype=np.float64).reshape(-1, 2)
n = len(k0)
np.random.seed(0)
v = ac.draw_mutations(args.gen, k0.shape)
obs = wh / wh.std(0)
index_sets = np.array([rs.choice(len(wh), n, replace=False) for _ in range(args.restarts)])
whd, vd = torch.from_numpy(wh).to(dev), torch.from_numpy(v).to(dev)
obsd = torch.from_numpy(obs).to(dev)


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t, r


def dev_evolve():
    kd = torch.from_numpy(k0.copy()).to(dev)
    f, acc = ops.anchor_evolve(whd, kd, vd, np.float32(0.25))
    return kd.cpu().numpy(), acc.cpu().numpy()


def dev_kmeans():
    codes = torch.from_numpy(obs[index_sets].astype(np.float64)).to(dev).contiguous()
    live = torch.ones(args.restarts, n, dtype=torch.int32, device=dev)
    dist = torch.zeros(args.restarts, dtype=torch.float64, device=dev)
    for _ in range(args.km_iters):
        ops.kmeans_step(obsd, codes, live, 0, dist)
        d = dist.cpu().numpy()
    return codes.cpu().numpy(), d


def host_kmeans():
    out = []
    o64 = obs.astype(np.float64)
    for idx in index_sets:
        book = o64[idx].copy()
        for _ in range(args.km_iters):
            d2 = ((o64[:, None, :] - book[None]) ** 2).sum(-1)
            code = d2.argmin(1)
            d = np.sqrt(d2[np.arange(len(o64)), code]).sum() / len(o64)
            cnt = np.bincount(code, minlength=n)
            book = np.stack([np.bincount(code, o64[:, 0], n), np.bincount(code, o64[:, 1], n)], 1) / np.maximum(cnt, 1)[:, None]
        out.append(d)
    return np.array(out)


arms = {
    "fitness": (lambda: anchor_metrics(whd, k0, 4.0)["fitness"], lambda: ac.fitness(wh, k0)),
    "evolve": (dev_evolve, lambda: ac.evolve(wh, k0, v)[:2]),
    "kmeans": (dev_kmeans, host_kmeans),
}
for d, _ in arms.values():   # warm-up: library load, workspace
    d()
times = {name: ([], []) for name in arms}
checks = {}
for _ in range(args.rounds):
    for name, (d, h) in arms.items():
        td, rd = timed(d)
        th, rh = timed(h)
        times[name][0].append(td)
        times[name][1].append(th)
        checks[name] = (rd, rh)
lines = [f"autoanchor A/B: {args.labels} labels, n = {n}, {args.rounds} interleaved rounds, {torch.cuda.get_device_name(0)}, {torch.get_num_threads()} host threads",
         f"evolve: {args.gen} generations; kmeans: {args.restarts} restarts x {args.km_iters} iterations", f"{'arm':10s} {'device ms':>12s} {'host ms':>12s} {'host / device':>14s}"]
for name, (td, th) in times.items():
    a, b = statistics.median(td) * 1e3, statistics.median(th) * 1e3
    lines.append(f"{name:10s} {a:12.3f} {b:12.3f} {b / a:14.1f}")
lines.append(f"agreement: fitness {abs(checks['fitness'][0] - checks['fitness'][1]):.3g}, evolve accepted equal {bool(np.array_equal(checks['evolve'][0][1], checks['evolve'][1][1]))}, "
             f"kmeans mean distance {float(np.abs(checks['kmeans'][0][1] - checks['kmeans'][1]).max()):.3g}")
report = "\n".join(lines)
print(report)
if args.out:
    Path(args.out).write_text(report + "\n")
