"""A/B of the optimizer step on yolov3's real parameter shapes, on one MI355X, in interleaved rounds:

  fused-adam   FusedAdam.step(grad_scale, max_norm, ema): unscale + inf check + clip + Adam + EMA lerp (csrc/optim.hip)
  torch-adam   what Adam cost before the fused step existed: torch.optim.Adam in each form the installed torch offers (fused=True, foreach=True) + clip_grad_norm_
               + ModelEMA's foreach lerp.  No unscale pass and no inf check are charged to it (GradScaler would add both, and a host sync).
  fused-sgd    FusedSGD.step with the same arguments: the existing step, measured in the same run

Every round times each arm `--iters` times with device events (median); the arms alternate within a round, so drift of the box hits all of them.  The condition
printed at the end: the fused Adam median is below the torch recipe's (its faster form) in EVERY round.  Achieved bytes per second are the algorithmic traffic
(Adam 36 B per element: gradient read, parameter / two moments / EMA read and written; SGD 28 B) over the median.

    python tools/optim_ab.py [--model yolov3] [--rounds 5] [--iters 20] [--out FILE]
"""
import argparse
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from yolov3_amd import DetectionModel  # noqa: E402
from yolov3_amd.optim import FusedAdam, FusedSGD, ModelEMA, smart_param_groups  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--model", default="yolov3")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--out", default=None, help="also write the report to this file")
args = ap.parse_args()
assert torch.cuda.is_available(), "optim_ab.py measures on an MI355X; there is nothing to measure without one"
dev = torch.device("cuda:0")
SCALE, MAX_NORM = 1024.0, 10.0


def model_with_grads(scale):
    """the model's parameters with gradients laid out as the training engine's backward does: slices of one flat arena, each 256-byte aligned"""
    m = DetectionModel(f"{args.model}.yaml").to(dev).train()
    ps = [p for p in m.parameters()]
    offs, o = [], 0
    for p in ps:
        offs.append(o)
        o += (p.numel() + 63) // 64 * 64
    arena = torch.randn(o, device=dev, generator=torch.Generator(dev).manual_seed(1)) * (1e-3 * scale)   # unscaled norm ~ 8: under max_norm
    for p, o in zip(ps, offs):
        p.grad = arena[o:o + p.numel()].view(p.shape)
    return m, ps


def fused_arm(cls, **kw):
    m, ps = model_with_grads(SCALE)
    opt = cls(smart_param_groups(m, 1e-3, 5e-4), **kw)
    ema = ModelEMA(m)
    return lambda: opt.step(grad_scale=SCALE, max_norm=MAX_NORM, ema=ema)


def torch_arm(**form):
    m, ps = model_with_grads(1.0)
    opt = torch.optim.Adam(smart_param_groups(m, 1e-3, 5e-4), **form)
    ema = ModelEMA(m)
    src = [p.detach() for p in ema.shadow] + list(ema.buffers)
    dst = list(ema.shadow.values()) + list(ema.buffers.values())

    def step():
        torch.nn.utils.clip_grad_norm_(ps, max_norm=MAX_NORM)
        opt.step()
        d = ema.next_decay()
        torch._foreach_mul_(dst, d)   # the foreach lerp over every parameter and float buffer (what ModelEMA ran before y3_ema_update: tools/ema_fold_pack_ab.py)
        torch._foreach_add_(dst, src, alpha=1.0 - d)

    return step


arms = {"fused-adam": fused_arm(FusedAdam), "fused-sgd": fused_arm(FusedSGD, momentum=0.937, nesterov=True)}
for name, form in (("torch-adam(fused=True)", {"fused": True}), ("torch-adam(foreach=True)", {"foreach": True})):
    try:
        step = torch_arm(**form)
        step()
        torch.cuda.synchronize()
        arms[name] = step
    except Exception as e:  # a form this torch build does not offer on this device
        print(f"{name}: not available here ({type(e).__name__}: {e})")
torch_names = [n for n in arms if n.startswith("torch-adam")]
assert torch_names, "no torch.optim.Adam form ran"
n_elem = sum(p.numel() for p in DetectionModel(f"{args.model}.yaml").parameters())


def timed(step, iters):
    ms = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        step()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms)


def kernel_launches(step):
    """device kernels of one step, counted by torch's profiler (memsets and copies not included)"""
    try:
        from torch.profiler import ProfilerActivity, profile

        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            step()
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if str(e.device_type).endswith("CUDA") and "memcpy" not in e.name.lower() and "memset" not in e.name.lower())
    except Exception as e:
        return f"not measured ({type(e).__name__})"


for step in arms.values():
    timed(step, args.warmup)
rounds = [{name: timed(step, args.iters) for name, step in arms.items()} for _ in range(args.rounds)]
launches = {name: kernel_launches(step) for name, step in arms.items()}

lines = [f"optimizer step A/B, {args.model} ({n_elem} parameter elements, {n_elem * 4 / 1e6:.0f} MB fp32), {args.rounds} interleaved rounds x {args.iters} steps, "
         f"median ms per round (device events), {torch.cuda.get_device_name(0)}, torch {torch.__version__}"]
for name in arms:
    per = [r[name] for r in rounds]
    bpe = 28 if name == "fused-sgd" else 36
    lines.append(f"{name:26s} rounds " + " ".join(f"{v:7.3f}" for v in per) + f"   median {statistics.median(per):7.3f} ms   kernels/step {launches[name]}   "
                 f"{n_elem * bpe / statistics.median(per) / 1e9:6.2f} TB/s of {bpe} B/element")
best_torch = [min(r[n] for n in torch_names) for r in rounds]
wins = [r["fused-adam"] < b for r, b in zip(rounds, best_torch)]
lines.append(f"fused-adam below the faster torch form in {sum(wins)} of {len(wins)} rounds: condition {'HOLDS' if all(wins) else 'DOES NOT HOLD'}; "
             f"ratio of medians {statistics.median(best_torch) / statistics.median(r['fused-adam'] for r in rounds):.2f}x")
report = "\n".join(lines)
print(report)
if args.out:
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(report + "\n")
