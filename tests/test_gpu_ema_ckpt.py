"""The EMA model on the MI355X: ModelEMA backed by a real module, half-precision inference plans straight from fp32 masters with ONE fold + pack launch
(y3_fold_pack_jobs), plan-cache version tracking for weights the kernels write behind torch's back, ema.update(model) (y3_ema_update), and the reference's checkpoint
round trip (save_checkpoint / attempt_load / smart_resume / strip_optimizer).

Shapes: yolov3-tiny and yolov3 at 64 x 64, batch 2.  Every comparison of two paths of this package is torch.equal: the kernels are deterministic and the new path is
built to repeat the old one's arithmetic operation for operation."""
import math
import subprocess
import sys
from copy import deepcopy
from pathlib import Path

import pytest
import torch
from torch import nn

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
HW, BS, NC = 64, 2, 80
MODELS = ["yolov3-tiny", "yolov3"]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


def randomise_bn(m, seed):
    """BatchNorm statistics and affine parameters away from their initial values, moderate enough that 75 layers of them keep the activations inside fp16's range
    (var 0.5 .. 2, gamma 1 +- 0.1); the extreme statistics (var 1e-6 .. 1e2) are the single-layer test's"""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, nn.BatchNorm2d):
                c = mod.num_features
                mod.running_var.copy_(2.0 ** (torch.rand(c, generator=g) * 2 - 1))
                mod.running_mean.copy_(torch.randn(c, generator=g) * 0.1)
                mod.weight.copy_(torch.randn(c, generator=g) * 0.1 + 1.0)
                mod.bias.copy_(torch.randn(c, generator=g) * 0.1)
    return m


_SD: dict = {}


def make(name, dev, nc=NC, seed=7):
    """a seeded fp32 model with randomised BatchNorm statistics (the state dict is computed once per (name, nc, seed) and never modified)"""
    from yolov3_amd import DetectionModel

    key = (name, nc, seed)
    m = DetectionModel(f"{name}.yaml", nc=nc)
    if key not in _SD:
        torch.manual_seed(seed)
        ref = DetectionModel(f"{name}.yaml", nc=nc)
        randomise_bn(ref, seed)
        _SD[key] = {k: v.clone() for k, v in ref.state_dict().items()}
    m.load_state_dict(_SD[key])
    return m.to(dev)


def image(dev, seed=5):
    return torch.rand(BS, 3, HW, HW, generator=torch.Generator().manual_seed(seed)).to(dev)


def run_eval(m, x):
    with torch.no_grad():
        pred, raw = m(x)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(pred).all())
    return [pred.clone()] + [r.clone() for r in raw]


def same(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and torch.equal(x, y) for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------------ 1. fold + pack bit parity
LAYERS = [(32, 3, 3, False, True), (64, 32, 3, False, True), (32, 64, 1, False, True), (255, 256, 1, True, False), (18, 128, 1, True, False), (1024, 512, 3, False, True)]


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float32], ids=["fp16", "bf16", "fp32"])
def test_fold_pack_jobs_equals_fold_and_pack_filter_bit_for_bit(dev, dtype):
    """(co, ci, k): the stem form, 3x3 and 1x1 layers, two Detect heads (bias, no BatchNorm; 255 and 18 filters: not multiples of 8), and a 1024 x 512 x 3 x 3 bank with
    its fragment-ordered copy -- all in ONE table launch, against engine._fold (torch arithmetic) + ops.pack_filter / pack_filter_stem per layer."""
    from yolov3_amd import engine, ops

    g = torch.Generator().manual_seed(31)
    jobs = engine.FoldPackJobs(dtype, dev)
    mods, got = [], []
    for i, (co, ci, k, bias, has_bn) in enumerate(LAYERS):
        conv = nn.Conv2d(ci, co, k, 1, k // 2, bias=bias)
        bn = nn.BatchNorm2d(co, eps=1e-3) if has_bn else None
        with torch.no_grad():
            conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) * 0.1)
            if bias:
                conv.bias.copy_(torch.randn(co, generator=g))
            if bn is not None:
                bn.running_var.copy_(10.0 ** (torch.rand(co, generator=g) * 8 - 6))   # 1e-6 .. 1e2
                bn.running_mean.copy_(torch.randn(co, generator=g))
                bn.weight.copy_(torch.randn(co, generator=g) + 1.0)
                bn.bias.copy_(torch.randn(co, generator=g))
        conv = conv.to(dev)
        bn = bn.to(dev).eval() if bn is not None else None
        stem = i == 0 and dtype != torch.float32   # (the stem kernel, and so its bank form, exists in f16 / bf16)
        mods.append((conv, bn, stem))
        got.append(jobs.add(conv, bn, True, stem=stem))
    jobs.run()
    torch.cuda.synchronize()
    assert not jobs.dirty
    for (conv, bn, stem), cw, (co, ci, k, _b, _n) in zip(mods, got, LAYERS):
        w, b = engine._fold(conv, bn)
        cout = (co + 7) // 8 * 8
        want = ops.pack_filter_stem(w, cout, dtype) if stem else ops.pack_filter(w, cout, (ci + 7) // 8 * 8, dtype)
        bias = torch.zeros(cout, dtype=torch.float32, device=dev)
        bias[:co] = b
        assert cw.filt.shape == want.shape and cw.filt.dtype == want.dtype
        bad = int((cw.filt != want).sum())
        assert torch.equal(cw.filt, want), f"bank of {(co, ci, k)}: {bad} of {want.numel()} elements differ"
        assert torch.equal(cw.bias, bias), f"bias of {(co, ci, k)}: max |diff| {float((cw.bias - bias).abs().max())}"
    # a second run after the weights moved refills the same banks
    ptr = got[1].filt.data_ptr()
    with torch.no_grad():
        mods[1][0].weight.mul_(-0.5)
    jobs.run()
    w, _ = engine._fold(mods[1][0], mods[1][1])
    assert got[1].filt.data_ptr() == ptr and torch.equal(got[1].filt, ops.pack_filter(w, 64, 32, dtype))


# ------------------------------------------------------------------------------------------------ 2. whole-model parity of the two paths
@pytest.mark.parametrize("name", MODELS)
def test_model_outputs_equal_under_both_fold_paths(dev, name, monkeypatch):
    from yolov3_amd import engine

    m = make(name, dev).eval()
    m.infer_dtype = torch.float16
    x = image(dev)
    monkeypatch.setenv("Y3_FOLD_PACK", "0")
    old = run_eval(m, x)
    assert all(f is None for f in engine.plan_cache(m).fold.values())
    m._drop_plans()
    monkeypatch.delenv("Y3_FOLD_PACK")
    new = run_eval(m, x)
    assert all(f is not None and len(f.jobs) > 0 for f in engine.plan_cache(m).fold.values())
    assert old[0].dtype == torch.float16 and next(m.parameters()).dtype == torch.float32
    assert same(old, new)
    # the switch is honoured without a dropped cache too
    monkeypatch.setenv("Y3_FOLD_PACK", "0")
    assert same(old, run_eval(m, x)) and all(f is None for f in engine.plan_cache(m).fold.values())
    # the parameters' own dtype still selects the plan dtype when infer_dtype is None
    monkeypatch.delenv("Y3_FOLD_PACK")
    m.infer_dtype = None
    assert run_eval(m, x)[0].dtype == torch.float32


# ------------------------------------------------------------------------------------------------ 3. version tracking
@pytest.mark.parametrize("name", MODELS)
def test_ema_plans_follow_the_fused_steps_without_a_rebuild(dev, name):
    from yolov3_amd import DetectionModel, FusedSGD, ModelEMA, engine, smart_param_groups

    m = make(name, dev).train()
    ema = ModelEMA(m)
    ema.ema.infer_dtype = torch.float16
    opt = FusedSGD(smart_param_groups(m, 0.01, 0.0), momentum=0.937, nesterov=True)
    x = image(dev)
    p0 = run_eval(ema.ema, x)
    builds = engine.EVAL_PLAN_BUILDS
    before = [e.clone() for e in ema.shadow.values()]
    g = torch.Generator().manual_seed(3)
    for _ in range(3):
        for p in m.parameters():   # a gradient of the weight's own size with random signs: every step moves a weight by ~2 % of itself
            p.grad = p.detach() * (torch.randint(0, 2, p.shape, generator=g).to(dev) * 2.0 - 1.0)
        opt.step(ema=ema)
    moved = [float(((e - b).abs().sum() / b.abs().sum().clamp_min(1e-12))) for e, b in zip(ema.shadow.values(), before) if b.numel() > 64]
    assert min(moved) >= 1e-2, min(moved)
    p1 = run_eval(ema.ema, x)
    assert engine.EVAL_PLAN_BUILDS == builds, "the eval plan of ema.ema was rebuilt"
    assert not torch.equal(p0[0], p1[0])
    fresh = DetectionModel(f"{name}.yaml", nc=NC).to(dev).eval()
    fresh.load_state_dict(ema.ema.state_dict())
    fresh.infer_dtype = torch.float16
    assert same(p1, run_eval(fresh, x))
    # the standalone update moves the version too
    with torch.no_grad():
        for p in m.parameters():
            p.mul_(1.5)
    ema.update(m)
    p2 = run_eval(ema.ema, x)
    assert engine.EVAL_PLAN_BUILDS == builds + 1 and not torch.equal(p1[0], p2[0])   # (+1: `fresh` compiled its own plan)
    fresh.load_state_dict(ema.ema.state_dict())
    assert same(p2, run_eval(fresh, x))


# ------------------------------------------------------------------------------------------------ 4. ema.update(model)
class Holder(nn.Module):
    def __init__(self, sizes, g):
        super().__init__()
        self.q = nn.ParameterList([nn.Parameter(torch.randn(n, generator=g)) for n in sizes])
        self.register_buffer("stat", torch.randn(37, generator=g))
        self.register_buffer("count", torch.tensor(5, dtype=torch.long))


def _ema_pair(kind, dev):
    """(model, ModelEMA whose averages differ from the model); built identically at every call"""
    from yolov3_amd import ModelEMA, freeze_layers

    g = torch.Generator().manual_seed(17)
    if kind == "holder":
        m = Holder([1, 16385, 100, 16384, 7], g).to(dev)   # 1 element; CHUNK + 1; exactly one chunk; odd sizes (tensors that start 4-byte aligned only)
    else:
        m = make("yolov3-tiny", dev, nc=3).train()
        freeze_layers(m, [2])
    ema = ModelEMA(m)
    with torch.no_grad():
        for v in ema.ema.state_dict().values():
            if v.dtype.is_floating_point:
                v.copy_((torch.randn(v.shape, generator=g) * 0.3).to(dev))
    return m, ema


@pytest.mark.parametrize("kind", ["holder", "frozen-tiny"])
@pytest.mark.parametrize("updates", [1, 2, 2001])
def test_ema_update_against_the_reference_arithmetic(dev, kind, updates):
    """upstream ModelEMA.update on the CPU, every operand and operation in fp32: v *= d; v += (1 - d) * m over every float entry of the state dict, against ONE
    y3_ema_update launch.  Bound per element: 2^-23 (|d v| + |(1 - d) m|), one fp32 rounding of either product (what contracting the final add could change)."""
    m, ema = _ema_pair(kind, dev)
    ema.updates = updates - 1
    msd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    want = {k: v.detach().cpu().clone() for k, v in ema.ema.state_dict().items()}
    d = torch.tensor(0.9999 * (1 - math.exp(-updates / 2000)), dtype=torch.float32)
    bound = {}
    for k, v in want.items():
        if v.dtype.is_floating_point:
            bound[k] = 2.0 ** -23 * ((d * v).abs() + ((1 - d) * msd[k]).abs())
            v *= d
            v += (1 - d) * msd[k]
    e0 = getattr(ema.ema, "weights_epoch", 0)
    ema.update(m)
    torch.cuda.synchronize()
    assert ema.updates == updates and ema.ema.weights_epoch == e0 + 1
    worst = 0.0
    for k, v in ema.ema.state_dict().items():
        got = v.detach().cpu()
        if not v.dtype.is_floating_point:
            assert torch.equal(got, want[k]), k   # integer entries (num_batches_tracked) are not averaged, as upstream
            continue
        err = (got - want[k]).abs()
        worst = max(worst, float((err / bound[k].clamp_min(1e-45)).max()))
        assert bool((err <= bound[k]).all()), (k, float(err.max()))
    print(f"ema.update {kind} updates={updates}: worst |hip - cpu| / bound = {worst:.3f}")
    assert all(torch.equal(v.detach().cpu(), msd[k]) for k, v in m.state_dict().items())   # the model is read only


@pytest.mark.parametrize("kind", ["holder", "frozen-tiny"])
def test_ema_update_equals_the_lerp_of_the_fused_step(dev, kind):
    """one definition of the lerp: a fused SGD step that leaves the parameters where they are (lr 0, zero gradients, no weight decay) applies to the averages what
    ema.update(model) applies -- the stepped parameters inside the SGD kernel, the frozen ones and the buffers through y3_ema_update"""
    from yolov3_amd import FusedSGD

    m1, ema1 = _ema_pair(kind, dev)
    m2, ema2 = _ema_pair(kind, dev)
    assert all(torch.equal(a, b) for a, b in zip(ema1.ema.state_dict().values(), ema2.ema.state_dict().values()))
    ema1.updates = ema2.updates = 2000
    params = [p for p in m1.parameters() if p.requires_grad]
    before = [p.detach().clone() for p in params]
    for p in params:
        p.grad = torch.zeros_like(p)
    opt = FusedSGD(params, lr=0.0, momentum=0.937, nesterov=True, weight_decay=0.0)
    opt.step(ema=ema1)
    ema2.update(m2)
    torch.cuda.synchronize()
    assert all(torch.equal(p.detach(), b) for p, b in zip(params, before)) and ema1.updates == ema2.updates == 2001
    if kind != "holder":
        assert 0 < len(params) < len(list(m1.parameters()))
    for (k, a), b in zip(ema1.ema.state_dict().items(), ema2.ema.state_dict().values()):
        assert torch.equal(a, b), k
    assert not torch.equal(next(iter(ema1.shadow.values())), next(iter(_ema_pair(kind, dev)[1].shadow.values())))   # (the averages did move)


# ------------------------------------------------------------------------------------------------ 5. checkpoint round trip
def train_step(m, opt, ema, x):
    opt.zero_grad()
    with torch.autocast("cuda", dtype=torch.float16):
        raws = m(x)
    g = torch.Generator().manual_seed(23)
    gs = [(torch.randn(r.shape, generator=g) * 0.01).to(r.device, r.dtype) for r in raws]
    torch.autograd.backward(list(raws), gs)
    opt.step(max_norm=10.0, ema=ema)
    torch.cuda.synchronize()


def test_checkpoint_round_trip(dev, tmp_path):
    """A checkpoint holds half copies (reference train.py:470-488), so a resumed run continues from the ROUNDED model and average.  To compare it with the run that
    wrote the checkpoint, that run is put on the checkpoint's values first (every float tensor rounded through half in place): from there the two must agree bit for bit."""
    from yolov3_amd import DetectionModel, ModelEMA, attempt_load, compat, save_checkpoint, smart_optimizer, smart_resume, strip_optimizer

    name = "yolov3-tiny"
    m = make(name, dev).train()
    opt = smart_optimizer(m, "SGD", lr=0.01, momentum=0.937, decay=5e-4)
    ema = ModelEMA(m)
    x = image(dev)
    train_step(m, opt, ema, x)
    with torch.no_grad():
        for md in (m, ema.ema):
            for v in md.state_dict().values():
                if v.dtype.is_floating_point:
                    v.copy_(v.half().float())
    ema.touched()
    f = tmp_path / "last.pt"
    save_checkpoint(f, m, ema, opt, epoch=0, best_fitness=0.1)
    assert all(p.dtype == torch.float32 for p in ema.ema.parameters())
    # what attempt_load returns runs like the averaged model cast to half
    direct = deepcopy(ema.ema).half()
    loaded = attempt_load(f, device=dev, fuse=False).half()
    assert same(run_eval(direct, x.half()), run_eval(loaded, x.half()))
    # resume into fresh objects
    ck = compat.load_checkpoint(f)
    m2 = DetectionModel(f"{name}.yaml", nc=NC)
    m2.load_state_dict(ck["model"].float().state_dict())
    m2 = m2.to(dev).train()
    opt2 = smart_optimizer(m2, "SGD", lr=0.5, momentum=0.1, decay=0.0)
    ema2 = ModelEMA(m2)
    assert smart_resume(ck, opt2, ema2, weights=str(f)) == (0.1, 1, 300)
    assert ema2.updates == ema.updates == 1
    train_step(m, opt, ema, x)
    train_step(m2, opt2, ema2, x)
    for (k, a), b in zip(m.state_dict().items(), m2.state_dict().values()):
        assert torch.equal(a, b), f"model {k}"
    for (k, a), b in zip(ema.ema.state_dict().items(), ema2.ema.state_dict().values()):
        assert torch.equal(a, b), f"ema {k}"
    s1, s2 = opt.state_dict(), opt2.state_dict()
    assert s1["param_groups"] == s2["param_groups"] and set(s1["state"]) == set(s2["state"]) and len(s1["state"]) > 0
    assert all(torch.equal(s1["state"][i]["momentum_buffer"], s2["state"][i]["momentum_buffer"]) for i in s1["state"])
    assert ema.updates == ema2.updates == 2
    # strip
    s = tmp_path / "best.pt"
    d = strip_optimizer(f, s)
    assert d["ema"] is None and d["optimizer"] is None and d["epoch"] == -1 and all(p.dtype == torch.float16 and not p.requires_grad for p in d["model"].parameters())
    stripped = attempt_load(s, device=dev, fuse=False).half()
    assert same(run_eval(loaded, x.half()), run_eval(stripped, x.half()))
    # a bare process (no reference on its path) loads the file and runs it
    code = f"""
import sys, torch
sys.path.insert(0, {str(ROOT)!r})
from yolov3_amd import compat, DetectionModel
m = compat.attempt_load({str(f)!r}, device='cuda:0')
assert type(m) is DetectionModel and not any(k == 'models' or k.startswith('models.') for k in sys.modules)
x = torch.rand(1, 3, 64, 64, device='cuda:0')
with torch.no_grad():
    pred = m(x)[0]
torch.cuda.synchronize()
assert pred.shape == (1, 3 * (4 * 4 + 2 * 2), 85) and bool(torch.isfinite(pred).all())
print('ok')
"""
    out = subprocess.run([sys.executable, "-c", code], cwd=tmp_path, text=True, capture_output=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr


# ------------------------------------------------------------------------------------------------ 6. validation of the averaged model in half precision
def test_run_batches_half_on_the_fp32_ema_model(dev):
    import numpy as np

    from yolov3_amd import ModelEMA, run_batches

    nc = 3
    m = make("yolov3-tiny", dev, nc=nc).train()
    ema = ModelEMA(m)
    g = torch.Generator().manual_seed(9)
    shapes = [((HW, HW), ((1.0, 1.0), (0.0, 0.0)))] * BS
    batches = []
    for _ in range(2):
        im = torch.rand(BS, 3, HW, HW, generator=g)
        t = torch.cat([torch.tensor([[float(i), float(c)]]).repeat(1, 1) for i in range(BS) for c in range(nc)], 0)
        box = torch.rand(t.shape[0], 4, generator=g) * 0.4 + 0.3
        batches.append((im, torch.cat([t, box], 1), shapes))
    with torch.no_grad():
        res, maps, st = run_batches(ema.ema, batches, nc=nc, half=True)
    assert "infer_dtype" not in ema.ema.__dict__ and ema.ema.infer_dtype is None
    assert all(p.dtype == torch.float32 for p in ema.ema.parameters()) and all(b.dtype != torch.float16 for b in ema.ema.buffers())
    byhand = deepcopy(ema.ema)
    byhand.infer_dtype = torch.float16
    with torch.no_grad():
        res2, maps2, st2 = run_batches(byhand, batches, nc=nc)
    assert res == res2 and np.array_equal(np.asarray(maps), np.asarray(maps2))
    # the forwards ran in half precision from fp32 masters; without the option the same model answers in fp32
    with torch.no_grad():
        assert ema.ema(batches[0][0].to(dev))[0].dtype == torch.float32 and byhand(batches[0][0].to(dev).half())[0].dtype == torch.float16
