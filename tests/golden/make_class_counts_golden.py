"""Generate tests/golden/class_counts.pt by running the UNMODIFIED reference (through oracle/ref_shim.py) at the class counts the other fixtures do not hold:
`ComputeLoss` (utils/loss.py:98-244) value, items and d loss / d p on yolov3-tiny heads with nc 1 / 2 and yolov3 heads with nc 1 / 3 / 60, and the eval branch of
`Detect` (models/yolo.py:98-110) for nc 1 / 2.  nc = 1 is the single-class case: the reference drops the class loss there (`if self.nc > 1`, :164).
Run where the reference tree is present:

    python tests/golden/make_class_counts_golden.py

The fixture stores reference OUTPUTS, the seeds and input checksums only; the tests regenerate the inputs from the seeds (oracle.yolo_oracle.synth_*)."""
from __future__ import annotations

import sys
from pathlib import Path

import torch
import yaml

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

from class_count_cases import pick_targets, scaled_hyp  # noqa: E402
from oracle import ref_shim, yolo_oracle as yo  # noqa: E402

OUT = Path(__file__).resolve().parent
CFG = ROOT / "yolov3_amd" / "cfg"

# (cfg, nc, image size, batch, hyp overrides)
LOSS_CASES = [
    ("yolov3-tiny", 1, 96, 2, {}),
    ("yolov3-tiny", 2, 96, 2, {}),
    ("yolov3-tiny", 2, 96, 2, dict(fl_gamma=1.5)),
    ("yolov3-tiny", 2, 96, 2, dict(label_smoothing=0.1)),
    ("yolov3-tiny", 2, 96, 2, dict(fl_gamma=1.5, label_smoothing=0.1)),
    ("yolov3", 1, 64, 2, {}),
    ("yolov3", 3, 64, 2, {}),
    ("yolov3", 60, 64, 2, {}),
]
# (nc, dtype): yolov3-tiny's Detect at 64 px (4 x 4 and 2 x 2 cells; the maps are one column wider, as make_golden.py's decode cases are), bs 2
DECODE_CASES = [(1, torch.float32), (1, torch.float16), (2, torch.float32), (2, torch.float16)]
TARGET_SEED0, PRED_SEED0, MODEL_SEED0, DECODE_SEED = 170, 150, 140, 23


def checksum(t: torch.Tensor) -> float:
    return float(t.double().abs().sum())


def _sparse(t: torch.Tensor) -> dict:
    """a mostly-zero tensor as (shape, flat indices of its non-zeros, their values)"""
    flat = t.reshape(-1)
    idx = flat.nonzero().reshape(-1)
    return {"shape": tuple(t.shape), "idx": idx.to(torch.int32), "val": flat[idx].clone()}


def _grad_record(g: torch.Tensor) -> dict:
    """d loss / d p of one level: the objectness plane (channel 4, dense: every cell has an objectness gradient) and the sparse rest (matched cells only)"""
    rest = g.clone()
    rest[..., 4] = 0
    return {"obj": g[..., 4].clone(), "rest": _sparse(rest)}


def gen_loss(ns):
    out = []
    for i, (name, nc, hw, bs, over) in enumerate(LOSS_CASES):
        layers, save, anchors, nc_v = yo.parse_cfg(yaml.safe_load(open(CFG / f"{name}.yaml")), 3, nc)
        strides = yo.model_strides(layers)
        sd = yo.seeded_state_dict(layers, nc_v, anchors, strides, seed=MODEL_SEED0 + i)
        m = ns.DetectionModel(str(CFG / f"{name}.yaml"), ch=3, nc=nc)
        m.load_state_dict(sd, strict=True)
        hyp = scaled_hyp(len(strides), nc, hw, over)
        m.hyp = hyp
        crit = ns.ComputeLoss(m)
        shapes = [(bs, 3, hw // int(s), hw // int(s), nc + 5) for s in strides]
        tg_seed, tg = pick_targets(bs, nc, shapes, m.model[-1].anchors, TARGET_SEED0 + 10 * i)
        p = [t.requires_grad_(True) for t in yo.synth_raw_predictions(shapes, seed=PRED_SEED0 + i)]
        loss, items = crit(p, tg)
        loss.backward()
        matched = [int((t.grad[..., :4].abs().sum(-1) > 0).sum()) for t in p]
        assert all(matched), f"case {i}: a level without a matched cell {matched}"
        out.append({"head": (name, nc, hw, bs), "over": over, "hyp": hyp, "anchors": m.model[-1].anchors.clone(), "tg_seed": tg_seed, "p_seed": PRED_SEED0 + i,
                    "tg_sum": checksum(tg), "p_sum": sum(checksum(t.detach()) for t in p), "loss": loss.detach().clone(), "items": items.detach().clone(),
                    "grads": [_grad_record(t.grad) for t in p]})
        print("loss", name, nc, hw, over, float(loss), items.tolist(), "targets", tg.shape[0], "matched cells", matched)
    return out


def gen_decode(ns):
    out = {}
    d = yaml.safe_load(open(CFG / "yolov3-tiny.yaml"))
    anchors, strides, sizes = d["anchors"], [16.0, 32.0], (4, 2)
    for nc, dtype in DECODE_CASES:
        no = nc + 5
        det = ns.Detect(nc, anchors, ch=(3 * no,) * 2)
        det.stride = torch.tensor(strides)
        det.anchors /= det.stride.view(-1, 1, 1)
        anchors_grid = det.anchors.clone().float()
        g = torch.Generator().manual_seed(DECODE_SEED)
        xs = [torch.randn(2, 3 * no, s, s + 1, generator=g) * 2.0 for s in sizes]
        if dtype == torch.float16:   # the decode lines in half on pre-rounded maps, the 1x1 convs out of the way (make_golden.py gen_decode_goldens)
            xs = [x.half().float() for x in xs]
            det.m = torch.nn.ModuleList(torch.nn.Identity() for _ in sizes)
            det.half()
            det.stride = det.stride.half()
            det.eval()
            with torch.no_grad():
                z, _ = det([x.half() for x in xs])
        else:
            for conv in det.m:
                conv.weight.data = torch.eye(3 * no).view(3 * no, 3 * no, 1, 1)
                conv.bias.data.zero_()
            det.eval()
            with torch.no_grad():
                z, _ = det([x.clone() for x in xs])
        out[f"nc{nc}-{str(dtype).split('.')[-1]}"] = {"sizes": sizes, "strides": strides, "anchors": anchors, "seed": DECODE_SEED, "in_sum": sum(checksum(x) for x in xs),
                                                       "z": z.clone(), "anchors_grid": anchors_grid}
        print("decode", nc, dtype, tuple(z.shape))
    return out


def main():
    torch.manual_seed(0)
    ns = ref_shim.load()
    out = {"loss": gen_loss(ns), "decode": gen_decode(ns)}
    torch.save(out, OUT / "class_counts.pt")
    print("class_counts.pt", (OUT / "class_counts.pt").stat().st_size, "bytes")


if __name__ == "__main__":
    main()
