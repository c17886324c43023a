"""A/B of the --multi-scale batch preparation on one MI355X, in interleaved rounds: the fused call (yolov3_amd.resize_batch: y3_resize_bilinear of
csrc/batch_edge.hip, one launch on the uint8 batch) against the torch sequence it replaces (reference train.py:380 + 399):

    imgs.float() / 255  ->  F.interpolate(imgs, size=ns, mode="bilinear", align_corners=False)  [-> .half() for fp16 output]

Batch 64 of uint8 640 x 640 to 320 / 640 / 960 squared, and the rect batch 384 x 640 to 448 x 704; fp32 and fp16 output.  Every shape of both arms is warmed up
first; then every round times each (case, dtype) once per arm, the arms alternating, with device events around `--iters` back-to-back calls.  Printed per case:
the median and the range of both arms, in how many rounds the fused arm was the faster one, its algorithmic bytes (the source read once, the output written once)
and their share of the HBM peak (bytes the call has to move over its time, not a traffic counter).  The fused form moves about a third or less of the torch
sequence's bytes: it has to be the faster arm in every round; the report says so when it is not, and the exit status is 1.

    python tools/multiscale_resize_ab.py [--batch 64] [--rounds 5] [--iters 10] [--out profiles/multiscale_resize_ab.txt]
"""
import argparse
import statistics
import sys
from pathlib import Path

import torch
import torch.nn.functional as F

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from yolov3_amd import resize_batch  # noqa: E402

HBM_PEAK = 8.0e12   # bytes / s, the MI355X's HBM3E specification (a float4 copy kernel reaches about 6.3e12 of it)

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--out", default=str(ROOT / "profiles" / "multiscale_resize_ab.txt"), help="the report is also written to this file ('' for none)")
args = ap.parse_args()
assert torch.cuda.is_available(), "multiscale_resize_ab.py measures on an MI355X; there is nothing to measure without one"
dev = torch.device("cuda:0")

CASES = [((640, 640), (320, 320)), ((640, 640), (640, 640)), ((640, 640), (960, 960)), ((384, 640), (448, 704))]
DTYPES = [torch.float32, torch.float16]
g = torch.Generator().manual_seed(0)
batches = {hw: torch.randint(0, 256, (args.batch, 3, *hw), generator=g, dtype=torch.uint8).to(dev) for hw in {c[0] for c in CASES}}


def fused(u, size, dt):
    return resize_batch(u, size, dtype=dt)


def torch_seq(u, size, dt):
    x = F.interpolate(u.float() / 255, size=size, mode="bilinear", align_corners=False)   # (the reference skips the interpolate at sf == 1; a drawn size never is)
    return x.half() if dt == torch.float16 else x


def timed(fn, *a):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.iters):
        fn(*a)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / args.iters   # ms per call


keys = [(src, size, dt) for src, size in CASES for dt in DTYPES]
agree = {}
for src, size, dt in keys:   # warm-up of every shape in both arms (library load, the allocator's blocks), and the agreement of the two arms
    a, b = fused(batches[src], size, dt), torch_seq(batches[src], size, dt)
    agree[(src, size, dt)] = (a.float() - b.float()).abs().max().item()
    del a, b
torch.cuda.synchronize()
times = {k: ([], []) for k in keys}
for r in range(args.rounds):
    for k in keys:
        src, size, dt = k
        arms = [(0, fused), (1, torch_seq)]
        for i, fn in (arms if r % 2 == 0 else arms[::-1]):   # the arm that goes first alternates from round to round
            times[k][i].append(timed(fn, batches[src], size, dt))

lines = [f"multi-scale resize A/B: batch {args.batch} uint8, {args.rounds} interleaved rounds x {args.iters} calls, device events, {torch.cuda.get_device_name(0)}",
         "fused = yolov3_amd.resize_batch (one launch); torch = .float() / 255, F.interpolate(bilinear), .half() for fp16; ms per call: median [min .. max]",
         "bytes = source read once + output written once (algorithmic, not measured traffic: a source read again in back-to-back calls may come from the 256 MiB Infinity Cache);",
         f"TB/s and share of the HBM peak of {HBM_PEAK / 1e12:.1f} TB/s = those bytes over the fused median",
         f"{'case':28s} {'out':5s} {'fused ms':>24s} {'torch ms':>24s} {'torch/fused':>11s} {'fused faster':>12s} {'MB':>8s} {'TB/s':>6s} {'of peak':>8s} {'max |diff|':>10s}"]
bad = []
for k in keys:
    src, size, dt = k
    tf, tt = times[k]
    mf, mt = statistics.median(tf), statistics.median(tt)
    wins = sum(1 for a, b in zip(tf, tt) if a < b)
    nbytes = args.batch * 3 * (src[0] * src[1] + size[0] * size[1] * (4 if dt == torch.float32 else 2))
    rate = nbytes / (mf * 1e-3)
    name = f"{src[0]}x{src[1]} -> {size[0]}x{size[1]}"
    lines.append(f"{name:28s} {'fp32' if dt == torch.float32 else 'fp16':5s} {f'{mf:.4f} [{min(tf):.4f} .. {max(tf):.4f}]':>24s} {f'{mt:.4f} [{min(tt):.4f} .. {max(tt):.4f}]':>24s} "
                 f"{mt / mf:11.2f} {f'{wins}/{len(tf)}':>12s} {nbytes / 1e6:8.1f} {rate / 1e12:6.2f} {100 * rate / HBM_PEAK:7.1f}% {agree[k]:10.2e}")
    if wins != len(tf):
        bad.append(name + (" fp32" if dt == torch.float32 else " fp16"))
lines.append("the fused arm was the faster one in every round of every case" if not bad else "DEFECT: the fused arm was not the faster one in every round of: " + ", ".join(bad))
report = "\n".join(lines)
print(report)
if args.out:
    Path(args.out).write_text(report + "\n")
sys.exit(1 if bad else 0)
