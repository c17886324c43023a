"""Checkpoint egress on the MI355X: save_reference_checkpoint on the LIVE device objects of a training loop -- yolov3-tiny nc=3, batch 2, 64 x 64, autocast fp16,
FusedSGD through GradScaler.step(..., ema=ema), ComputeLoss over a handful of targets -- after two optimizer steps.  The file carries the reference's class names
only, loads back here onto the device and runs like the averaged model, resumes bit for bit, and writing it leaves the plans, the filter banks and the arena of the
live model alone: a third step gives the loss and the gradients of a twin that never exported.

No reference tree is read (tests/test_reference_export_cpu.py loads such files in the unmodified reference).  Every comparison is torch.equal: both sides run the
same deterministic kernels on the same bits."""
import pickletools
import zipfile
from copy import deepcopy

import pytest
import torch
from torch import nn

pytestmark = pytest.mark.gpu

HW, BS, NC = 64, 2, 3
HYP = dict(box=0.05, cls=0.5, cls_pw=1.0, obj=1.0, obj_pw=1.0, anchor_t=4.0, fl_gamma=0.0, label_smoothing=0.0)
NAMES = {0: "cat", 1: "dog", 2: "emu"}
#                        img cls  x     y     w     h
TARGETS = torch.tensor([[0, 0, 0.30, 0.35, 0.20, 0.30],
                        [0, 2, 0.70, 0.60, 0.45, 0.40],
                        [0, 1, 0.52, 0.48, 0.10, 0.12],
                        [1, 1, 0.25, 0.75, 0.30, 0.25],
                        [1, 0, 0.80, 0.20, 0.15, 0.22]], dtype=torch.float32)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


def _state_dict():
    from yolov3_amd import DetectionModel

    torch.manual_seed(7)
    m = DetectionModel("yolov3-tiny.yaml", nc=NC)
    g = torch.Generator().manual_seed(7)
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, nn.BatchNorm2d):
                c = mod.num_features
                mod.running_var.copy_(2.0 ** (torch.rand(c, generator=g) * 2 - 1))
                mod.running_mean.copy_(torch.randn(c, generator=g) * 0.1)
                mod.weight.copy_(torch.randn(c, generator=g) * 0.1 + 1.0)
                mod.bias.copy_(torch.randn(c, generator=g) * 0.1)
    return {k: v.clone() for k, v in m.state_dict().items()}


class Loop:
    """the objects of one training run and its step (reference train.py:401-422)"""

    def __init__(self, sd, dev):
        from yolov3_amd import ComputeLoss, DetectionModel, FusedSGD, GradScaler, ModelEMA, smart_param_groups

        m = DetectionModel("yolov3-tiny.yaml", nc=NC)
        m.load_state_dict(sd)
        self.m = m.to(dev).train()
        self.m.nc, self.m.hyp, self.m.names = NC, dict(HYP), dict(NAMES)
        self.crit = ComputeLoss(self.m)
        self.opt = FusedSGD(smart_param_groups(self.m, 0.01, 5e-4), momentum=0.937, nesterov=True)
        self.ema = ModelEMA(self.m)
        self.scaler = GradScaler(init_scale=1024.0)
        self.dev = dev

    def step(self, i):
        x = torch.rand(BS, 3, HW, HW, generator=torch.Generator().manual_seed(40 + i)).to(self.dev)
        with torch.autocast("cuda", dtype=torch.float16):
            loss, items = self.crit(self.m(x), TARGETS.to(self.dev))
        self.scaler.scale(loss).backward()
        grads = [p.grad.clone() for p in self.m.parameters()]
        self.scaler.unscale_(self.opt)
        self.scaler.step(self.opt, max_norm=10.0, ema=self.ema)
        self.scaler.update()
        self.opt.zero_grad()
        torch.cuda.synchronize()
        return loss.detach().clone(), items.detach().clone(), grads


@pytest.fixture(scope="module")
def run(dev, tmp_path_factory):
    """two steps on two identical runs, the export from one of them, a third step on both; computed once"""
    from yolov3_amd import save_reference_checkpoint

    sd = _state_dict()
    a, b = Loop(sd, dev), Loop(sd, dev)
    first = [(a.step(i), b.step(i)) for i in range(2)]
    held = {"model": {k: v.detach().clone() for k, v in a.m.state_dict().items()}, "ema": {k: v.detach().clone() for k, v in a.ema.ema.state_dict().items()},
            "state": {k: a.opt.state[p].clone() for k, p in a.m.named_parameters()}, "updates": a.ema.updates,
            "ids": [id(x) for x in a.m.modules()] + [id(p) for p in a.m.parameters()]}
    f = tmp_path_factory.mktemp("gpu_export") / "last.pt"
    ck = save_reference_checkpoint(f, a.m, a.ema, a.opt, epoch=0, best_fitness=0.1)
    third = (a.step(2), b.step(2))
    return {"a": a, "b": b, "first": first, "third": third, "held": held, "f": f, "ck": ck}


def _equal_steps(s, t):
    return torch.equal(s[0], t[0]) and torch.equal(s[1], t[1]) and len(s[2]) == len(t[2]) and all(torch.equal(g, h) for g, h in zip(s[2], t[2]))


def test_the_loop_stepped_and_the_twins_agree_before_the_export(run):
    assert run["held"]["updates"] == 2 and all(_equal_steps(s, t) for s, t in run["first"])
    assert all(bool(torch.isfinite(s[0]).all()) and all(bool(torch.isfinite(g).all()) and bool(g.any()) for g in s[2]) for s, _ in run["first"])
    assert len(run["held"]["state"]) == len(list(run["a"].m.parameters())) and all(bool(v.any()) for v in run["held"]["state"].values())


def test_stream_holds_reference_names_only(run):
    from yolov3_amd import common, compat

    with zipfile.ZipFile(run["f"]) as z:
        data = z.read(next(n for n in z.namelist() if n.endswith("/data.pkl")))
    found = set()
    for op, arg, _ in pickletools.genops(data):
        if isinstance(arg, str):
            assert not arg.startswith("yolov3_amd"), f"{op.name} {arg!r}"
        assert op.name != "STACK_GLOBAL"   # torch.save's protocol 2 writes GLOBAL, which carries both strings
        if op.name == "GLOBAL":
            found.add(tuple(arg.split(" ", 1)))
    ours = {n for n in found if n[0].startswith("models")}
    assert ours == {("models.yolo", "DetectionModel"), ("models.yolo", "Detect"), ("models.common", "Conv"), ("models.common", "Concat")} and ours <= set(compat._class_map())
    ck = run["ck"]
    assert all(p.dtype == torch.float16 and p.is_cuda for k in ("model", "ema") for p in ck[k].parameters())
    for k in ("model", "ema"):
        kinds = {type(x) for x in ck[k].model}
        assert kinds >= {nn.Upsample, nn.MaxPool2d, nn.ZeroPad2d} and not kinds & {common.Upsample, common.MaxPool2d, common.ZeroPad2d}
        assert all(isinstance(g, list) and len(g) == 2 for g in (ck[k].model[-1].grid, ck[k].model[-1].anchor_grid))


def test_the_export_left_the_live_objects_alone(run):
    a, held = run["a"], run["held"]
    assert [id(x) for x in a.m.modules()] + [id(p) for p in a.m.parameters()] == held["ids"]
    assert all(p.dtype == torch.float32 and p.requires_grad for p in a.m.parameters()) and not hasattr(a.m.model[-1], "grid")
    # a third step on the live model: the loss and the gradients of the twin that never exported, then the same weights, averages and momenta
    assert _equal_steps(*run["third"])
    b = run["b"]
    assert a.ema.updates == b.ema.updates == 3
    for x, y in ((a.m, b.m), (a.ema.ema, b.ema.ema)):
        assert all(torch.equal(v, w) for v, w in zip(x.state_dict().values(), y.state_dict().values()))
    assert all(torch.equal(a.opt.state[p], b.opt.state[q]) for p, q in zip(a.m.parameters(), b.m.parameters()))


def test_the_file_loads_on_the_device_and_runs_like_the_averaged_model(run, dev):
    """A checkpoint holds HALF copies (reference train.py:470-488), so what comes back is the averaged model rounded through half: the comparand is a copy of ema.ema
    as it stood at the export with every float entry rounded the same way (as tests/test_gpu_ema_ckpt.py::test_checkpoint_round_trip puts it).  Both then run in half
    precision from fp32 masters (infer_dtype), unfused, so the engine folds and packs the same numbers."""
    from yolov3_amd import DetectionModel, attempt_load

    loaded = attempt_load(run["f"], device=dev, fuse=False)
    assert type(loaded) is DetectionModel and not loaded.training and all(p.dtype == torch.float32 and p.is_cuda for p in loaded.parameters())
    assert loaded.names == NAMES and loaded.hyp == HYP and loaded.nc == NC and loaded.stride.tolist() == [16.0, 32.0]
    want = deepcopy(run["a"].ema.ema)
    want.load_state_dict({k: v.half().float() if v.is_floating_point() else v for k, v in run["held"]["ema"].items()})
    assert all(torch.equal(v, w) for v, w in zip(loaded.state_dict().values(), want.state_dict().values()))
    loaded.infer_dtype = want.infer_dtype = torch.float16
    x = torch.rand(BS, 3, HW, HW, generator=torch.Generator().manual_seed(99)).to(dev).half()
    with torch.no_grad():
        p, q = loaded(x), want.eval()(x)
        fused = attempt_load(run["f"], device=dev)(x.float())[0]   # the default: fused, fp32
    torch.cuda.synchronize()
    assert p[0].dtype == torch.float16 and p[0].shape == (BS, 3 * (4 * 4 + 2 * 2), NC + 5) and bool(torch.isfinite(p[0]).all())
    assert torch.equal(p[0], q[0]) and all(torch.equal(r, s) for r, s in zip(p[1], q[1]))
    assert fused.shape == p[0].shape and bool(torch.isfinite(fused).all())


def test_resume_restores_state_and_updates_bit_for_bit(run, dev):
    from yolov3_amd import DetectionModel, FusedSGD, ModelEMA, compat, smart_param_groups, smart_resume

    ck = compat.load_checkpoint(run["f"])
    held = run["held"]
    assert all(torch.equal(v.to(dev), held["model"][k].half() if v.is_floating_point() else held["model"][k]) for k, v in ck["model"].state_dict().items())
    m2 = DetectionModel("yolov3-tiny.yaml", nc=NC)
    m2.load_state_dict(ck["model"].float().state_dict())
    m2 = m2.to(dev).train()
    opt2 = FusedSGD(smart_param_groups(m2, 0.5, 0.0), momentum=0.1, nesterov=False)
    ema2 = ModelEMA(m2)
    assert smart_resume(ck, opt2, ema2, weights=str(run["f"])) == (0.1, 1, 300)
    assert ema2.updates == held["updates"] == 2 and opt2.momentum == 0.937 and opt2.nesterov is True
    assert [(g["lr"], g["weight_decay"]) for g in opt2.param_groups] == [(0.01, 0.0), (0.01, 5e-4), (0.01, 0.0)]
    for k, p in m2.named_parameters():
        assert opt2.state[p].is_cuda and torch.equal(opt2.state[p], held["state"][k]), k
    for k, v in ema2.ema.state_dict().items():
        assert torch.equal(v, held["ema"][k].half().float() if v.is_floating_point() else held["ema"][k]), k
