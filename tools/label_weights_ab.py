"""A/B of the --image-weights epoch prologue at COCO scale on one MI355X, in interleaved rounds: the device calls (csrc/label_weights.hip through
yolov3_amd/label_weights.py) against the host form the reference runs (utils/general.py:543-568, train.py:333,360-363), written here with NumPy: one np.bincount
per image and random.choices.  Synthetic labels: --images images, --labels labels, nc classes.

  table          LabelTable(labels, nc): concatenate, upload, histogram, one read -- the one-off cost of the device form (the host form has none)
  class_weights  labels_to_class_weights: host concatenate + bincount + tail            device: the cached histogram + the same tail
  image_weights  labels_to_image_weights(labels, nc, cw)                                device: y3_image_weights and the read of n doubles
  epoch          cw, iw, random.choices(range(n), weights=iw, k=n) -- train.py:360-363  device: image_weight_indices (k random.random() draws on the host, two
                 uploads, y3_image_weights + y3_weighted_choices, one read of k + 1 words)

Every round times each arm once, the arms alternate within a round; medians over the rounds and the ratio host / device are printed.  No speed-up is promised:
the report records what was measured.  Run on the GPU machine under one time limit:

    timeout -k 10 600 python tools/label_weights_ab.py [--images 120000] [--labels 860000] [--nc 80] [--rounds 5] [--out profiles/label_weights_ab.txt]
"""
import argparse
import random
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from yolov3_amd import LabelTable, image_weight_indices, labels_to_class_weights, labels_to_image_weights  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--images", type=int, default=120_000)
ap.add_argument("--labels", type=int, default=860_000)
ap.add_argument("--nc", type=int, default=80)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--out", default=str(ROOT / "profiles" / "label_weights_ab.txt"), help="the report is also written to this file ('' for none)")
args = ap.parse_args()
assert torch.cuda.is_available(), "label_weights_ab.py measures on an MI355X; there is nothing to measure without one"
dev = torch.device("cuda:0")
nc, n = args.nc, args.images

rs = np.random.RandomState(0)
counts = rs.multinomial(args.labels, np.full(n, 1.0 / n))
popularity = rs.dirichlet(np.full(nc, 0.5))   # unbalanced classes, as in a real dataset
labels = [np.concatenate([rs.choice(nc, m, p=popularity)[:, None].astype(np.float64), rs.uniform(0.05, 0.95, (m, 4))], 1).astype(np.float32) for m in counts]
maps = rs.uniform(0.0, 1.0, nc)


def host_class_weights(labels, nc):
    cl = np.concatenate(labels, 0)
    weights = np.bincount(cl[:, 0].astype(int), minlength=nc)
    weights[weights == 0] = 1
    weights = 1 / weights
    weights /= weights.sum()
    return torch.from_numpy(weights).float()


def host_image_weights(labels, nc, class_weights):
    class_counts = np.array([np.bincount(x[:, 0].astype(int), minlength=nc) for x in labels])
    return (class_weights.reshape(1, nc) * class_counts).sum(1)


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t, r


table = LabelTable(labels, nc, dev)   # warm-up: library load, allocator
class_weights = labels_to_class_weights(table) * nc
cw = class_weights.numpy() * (1 - maps) ** 2 / nc


def host_epoch():
    random.seed(0)
    c = class_weights.numpy() * (1 - maps) ** 2 / nc
    iw = host_image_weights(labels, nc, c)
    return random.choices(range(n), weights=iw, k=n)


def dev_epoch():
    random.seed(0)
    c = class_weights.numpy() * (1 - maps) ** 2 / nc
    return image_weight_indices(table, c)


arms = {
    "table": (lambda: LabelTable(labels, nc, dev), lambda: None),
    "class_weights": (lambda: labels_to_class_weights(table), lambda: host_class_weights(labels, nc)),
    "image_weights": (lambda: labels_to_image_weights(table, nc, cw), lambda: host_image_weights(labels, nc, cw)),
    "epoch": (dev_epoch, host_epoch),
}
dev_epoch()   # warm-up: workspace
times = {name: ([], []) for name in arms}
checks = {}
for _ in range(args.rounds):
    for name, (d, h) in arms.items():
        td, rd = timed(d)
        th, rh = timed(h)
        times[name][0].append(td)
        times[name][1].append(th)
        checks[name] = (rd, rh)
lines = [f"label weights A/B: {n} images, {table.N} labels, nc = {nc}, {args.rounds} interleaved rounds, {torch.cuda.get_device_name(0)}, {torch.get_num_threads()} host threads",
         f"{'arm':14s} {'device ms':>12s} {'host ms':>12s} {'host / device':>14s}"]
for name, (td, th) in times.items():
    a, b = statistics.median(td) * 1e3, statistics.median(th) * 1e3
    lines.append(f"{name:14s} {a:12.3f} {b:12.3f} " + (f"{b / a:14.1f}" if name != "table" else f"{'(one-off)':>14s}"))
iw_d, iw_h = checks["image_weights"]
lines.append(f"agreement: class weights equal {bool(torch.equal(*checks['class_weights']))}, image weights largest relative gap {float((np.abs(iw_d - iw_h) / iw_h.clip(1e-300)).max()):.3g}, "
             f"indices differing {sum(a != b for a, b in zip(*checks['epoch']))} of {n}")
report = "\n".join(lines)
print(report)
if args.out:
    Path(args.out).write_text(report + "\n")
