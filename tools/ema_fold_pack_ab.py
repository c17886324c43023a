"""A/B of the two plan-time costs of validating a moving EMA model, on one MI355X, in interleaved rounds (device events, median per round):

  (a) refreshing every inference bank of the model (fp16 plans from fp32 masters) after a weight change:
        per-layer   Y3_FOLD_PACK=0: the plans are dropped, every layer is folded with torch arithmetic and packed by its own y3_pack_filter launch, the plan recompiled
        one-launch  the default: y3_fold_pack_jobs refills the existing banks
      Both arms are timed from the version bump to the end of the refresh and EXCLUDE the forward itself (the forward of the same plan is timed alone and subtracted).
  (b) ModelEMA.update(model) over the full float state:
        foreach     torch._foreach_mul_ + torch._foreach_add_ over every float entry (what update_buffers + update_rest ran before)
        one-launch  y3_ema_update

    python tools/ema_fold_pack_ab.py [--model yolov3] [--rounds 5] [--iters 10] [--out FILE]
"""
import argparse
import os
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from yolov3_amd import DetectionModel, ModelEMA  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--model", default="yolov3")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--hw", type=int, default=64)
ap.add_argument("--out", default=None, help="also write the report to this file")
args = ap.parse_args()
assert torch.cuda.is_available(), "ema_fold_pack_ab.py measures on an MI355X; there is nothing to measure without one"
dev = torch.device("cuda:0")
x = torch.rand(1, 3, args.hw, args.hw, device=dev)


def timed(fn, iters):
    ms = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms)


def refresh_arm(flag):
    m = DetectionModel(f"{args.model}.yaml").to(dev).eval()
    m.infer_dtype = torch.float16

    def forward():
        os.environ["Y3_FOLD_PACK"] = flag
        with torch.no_grad():
            m(x)

    def refresh_and_forward():
        m.weights_epoch += 1   # what a ModelEMA update does to its model
        forward()

    return forward, refresh_and_forward


def ema_arm(kind):
    m = DetectionModel(f"{args.model}.yaml").to(dev).train()
    ema = ModelEMA(m)
    msd, esd = m.state_dict(), ema.ema.state_dict()
    src = [msd[k] for k, v in esd.items() if v.dtype.is_floating_point]
    dst = [v for v in esd.values() if v.dtype.is_floating_point]

    def foreach():
        d = ema.next_decay()
        torch._foreach_mul_(dst, d)
        torch._foreach_add_(dst, src, alpha=1.0 - d)

    return foreach if kind == "foreach" else (lambda: ema.update(m))


arms = {}
for name, flag in (("refresh per-layer", "0"), ("refresh one-launch", "1")):
    fwd, ref = refresh_arm(flag)
    arms[name + " (forward alone)"] = fwd
    arms[name + " (+ forward)"] = ref
arms["ema foreach"] = ema_arm("foreach")
arms["ema one-launch"] = ema_arm("kernel")
for fn in arms.values():
    timed(fn, 3)
rounds = [{name: timed(fn, args.iters) for name, fn in arms.items()} for _ in range(args.rounds)]
os.environ.pop("Y3_FOLD_PACK", None)

n_elem = sum(v.numel() for v in DetectionModel(f"{args.model}.yaml").state_dict().values() if v.dtype.is_floating_point)
lines = [f"EMA validation plan-time A/B, {args.model} ({n_elem} float state elements), input 1 x 3 x {args.hw} x {args.hw}, {args.rounds} interleaved rounds x {args.iters} calls, "
         f"median ms per round (device events, host time of the call included), {torch.cuda.get_device_name(0)}, torch {torch.__version__}"]
for name in arms:
    per = [r[name] for r in rounds]
    lines.append(f"{name:40s} rounds " + " ".join(f"{v:8.3f}" for v in per) + f"   median {statistics.median(per):8.3f} ms")
for pair in ("refresh per-layer", "refresh one-launch"):
    net = [r[pair + " (+ forward)"] - r[pair + " (forward alone)"] for r in rounds]
    lines.append(f"{pair + ' net of the forward':40s} rounds " + " ".join(f"{v:8.3f}" for v in net) + f"   median {statistics.median(net):8.3f} ms")
a = [r["refresh one-launch (+ forward)"] < r["refresh per-layer (+ forward)"] for r in rounds]
b = [r["ema one-launch"] < r["ema foreach"] for r in rounds]
lines.append(f"(a) the one-launch refresh is below the per-layer path in {sum(a)} of {len(a)} rounds; (b) y3_ema_update is below the foreach lerp in {sum(b)} of {len(b)} rounds")
report = "\n".join(lines)
print(report)
if args.out:
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(report + "\n")
