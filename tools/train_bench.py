"""Phase timing of one training step (forward / loss / backward) on MI355X.  Not the driver's bench (bench.py keeps
BASELINE configs[1]); this is the measurement for the training half of the path (configs[2] per-GPU shape)."""
import argparse, json, sys, time
from pathlib import Path
import torch
sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from oracle import yolo_oracle as yo
from yolov3_amd import ComputeLoss, DetectionModel, _lib, freeze_layers

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=16)
ap.add_argument("--imgsz", type=int, default=640)
ap.add_argument("--steps", type=int, default=3)
ap.add_argument("--model", default="yolov3")
ap.add_argument("--fused", action="store_true")
ap.add_argument("--optimizer", choices=["SGD", "Adam", "AdamW", "RMSProp"], default="SGD", help="the reference's --optimizer; with --fused the fused step of that family (smart_optimizer)")
ap.add_argument("--freeze", type=int, nargs="+", default=[0], help="the reference's --freeze (train.py:217): [n] = layers 0 .. n-1 (10: the yolov3 backbone), a longer list names layers")
ap.add_argument("--launches", action="store_true", help="one more step under _lib.CallTimer: calls and milliseconds per C function, forward and backward")
args = ap.parse_args()
dev = torch.device("cuda:0")
m = DetectionModel(f"{args.model}.yaml").to(dev).train()
frozen = freeze_layers(m, args.freeze)
m.hyp = dict(box=0.05, cls=0.5, cls_pw=1.0, obj=1.0, obj_pw=1.0, anchor_t=4.0, fl_gamma=0.0, label_smoothing=0.0)
crit = ComputeLoss(m)
from yolov3_amd.optim import FusedSGD, ModelEMA, smart_optimizer, smart_param_groups
if args.fused:
    opt = FusedSGD(smart_param_groups(m, 0.01, 5e-4), momentum=0.937, nesterov=True) if args.optimizer == "SGD" else smart_optimizer(m, args.optimizer, 0.001, 0.937, 5e-4)
    ema = ModelEMA(m)
elif args.optimizer == "SGD":
    opt = torch.optim.SGD([p_ for p_ in m.parameters() if p_.requires_grad], lr=0.01, momentum=0.937, nesterov=True)
else:
    live = [p_ for p_ in m.parameters() if p_.requires_grad]
    opt = {"Adam": torch.optim.Adam, "AdamW": torch.optim.AdamW, "RMSProp": torch.optim.RMSprop}[args.optimizer](live, lr=0.001)
x = torch.rand(args.batch, 3, args.imgsz, args.imgsz, device=dev)
tg = yo.synth_targets(args.batch, 80, seed=1).to(dev)
def sync(): torch.cuda.synchronize(); return time.perf_counter()
res = []
for it in range(args.steps + 1):
    t0 = sync()
    with torch.autocast("cuda", dtype=torch.float16):
        raws = m(x)
        t1 = sync()
        loss, items = crit(raws, tg)
    t2 = sync()
    (loss * 1024.0).backward()
    t3 = sync()
    if args.fused:
        opt.step(grad_scale=1024.0, max_norm=10.0, ema=ema); opt.zero_grad()
    else:
        for p_ in m.parameters():
            if p_.grad is not None:
                p_.grad.div_(1024.0)  # GradScaler.unscale_
        opt.step(); opt.zero_grad(set_to_none=True)
    t4 = sync()
    if it:
        res.append((t1 - t0, t2 - t1, t3 - t2, t4 - t3))
f, l, b, o = (sum(r[i] for r in res) / len(res) * 1e3 for i in range(4))
tot = f + l + b + o
launches = None
if args.launches:
    launches = {}
    with torch.autocast("cuda", dtype=torch.float16):
        with _lib.CallTimer() as t_f:
            raws = m(x)
        launches["forward"] = {k: [round(v[0], 3), v[1]] for k, v in sorted(t_f.by_function().items())}
        loss, items = crit(raws, tg)
    with _lib.CallTimer() as t_b:
        (loss * 1024.0).backward()
    launches["backward"] = {k: [round(v[0], 3), v[1]] for k, v in sorted(t_b.by_function().items())}
    opt.zero_grad()
print(json.dumps({"workload": f"{args.model} train step {args.imgsz}x{args.imgsz} batch={args.batch} autocast fp16 (fwd BN batch stats + ComputeLoss + bwd + torch SGD)",
                  "ms": {"forward": round(f, 2), "loss": round(l, 2), "backward": round(b, 2), (f"optimizer(fused {args.optimizer.lower()}+clip+ema)" if args.fused else f"optimizer(torch {args.optimizer.lower()})"): round(o, 2), "total": round(tot, 2)},
                  "steps_ms": [round(sum(r) * 1e3, 2) for r in res], "freeze": args.freeze, "frozen_parameters": len(frozen),
                  "live_parameter_elements": sum(p_.numel() for p_ in m.parameters() if p_.requires_grad),
                  "images_per_sec": round(args.batch / tot * 1e3, 1), "loss": float(loss), **({"launches_ms_calls": launches} if launches else {})}))
