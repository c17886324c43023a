"""Frozen-layer training on the MI355X (yolov3_amd.freeze_layers + the training engine's need analysis): a step with frozen layers computes, bit for bit, what the
unfrozen step computes for everything that is still trained -- the same deterministic kernels run on the same operands, so every comparison is
torch.equal -- leaves the frozen parameters without a gradient, and really skips their backward launches.

Shapes: 64 x 64, batch 2 (every unit kind of the three models: MaxPool / ZeroPad / Upsample in yolov3-tiny; shortcuts with deferred gradients, stride-2 data gradients and
Concat slices in yolov3; the SPP unit in yolov3-spp).  Weights are seeded, the upstream gradient is a fixed seeded tensor per head (the loss kernels are not under test).
A layer list of ONE element means range(n) (reference train.py:217), so a single layer is named twice: [4, 4] freezes layer 4 alone."""
import contextlib
from pathlib import Path

import pytest
import torch
import yaml

from oracle import yolo_oracle as yo

pytestmark = pytest.mark.gpu

CFG = Path(__file__).resolve().parents[1] / "yolov3_amd" / "cfg"
HW, BS, NC = 64, 2, 80


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


_SD: dict = {}
_REF: dict = {}


def seeded_sd(name):
    if name not in _SD:
        d = yaml.safe_load(open(CFG / f"{name}.yaml"))
        layers, save, anchors, nc_v = yo.parse_cfg(d, 3, NC)
        _SD[name] = yo.seeded_state_dict(layers, nc_v, anchors, yo.model_strides(layers), seed=11)
    return _SD[name]


def make(name, dev, sd=None):
    from yolov3_amd import DetectionModel

    m = DetectionModel(f"{name}.yaml", nc=NC)
    m.load_state_dict(sd if sd is not None else seeded_sd(name))
    return m.to(dev).train()


def image(dev, seed=5):
    return torch.rand(BS, 3, HW, HW, generator=torch.Generator().manual_seed(seed)).to(dev)


def step(m, x, dtype):
    """one forward + backward under the fixed upstream gradient; returns the forward outputs (clones)"""
    m.zero_grad(set_to_none=True)
    ctx = torch.autocast("cuda", dtype=dtype) if dtype != torch.float32 else contextlib.nullcontext()
    with ctx:
        raws = m(x)
    outs = [r.detach().clone() for r in raws]
    g = torch.Generator().manual_seed(23)
    gs = [(torch.randn(r.shape, generator=g) * 0.01).to(r.device, r.dtype) for r in raws]
    torch.autograd.backward(list(raws), gs)
    torch.cuda.synchronize()
    return outs


def snapshot(m, outs):
    return {"out": outs, "grad": {k: (None if p.grad is None else p.grad.clone()) for k, p in m.named_parameters()},
            "buf": {k: b.clone() for k, b in m.named_buffers()}}


def unfrozen(name, dtype, dev):
    """the unfrozen step of (model, dtype) from the seeded weights: computed once, shared, never modified"""
    key = (name, dtype)
    if key not in _REF:
        m = make(name, dev)
        _REF[key] = snapshot(m, step(m, image(dev), dtype))
        assert all(g is not None and bool(torch.isfinite(g).all()) for g in _REF[key]["grad"].values())
    return _REF[key]


def check_against_unfrozen(m, got, ref):
    live = 0
    for k, p in m.named_parameters():
        if p.requires_grad:
            live += 1
            assert got["grad"][k] is not None and torch.equal(got["grad"][k], ref["grad"][k]), f"gradient of {k}"
        else:
            assert got["grad"][k] is None, f"{k} is frozen and has a gradient"
    assert 0 < live < len(got["grad"])
    for k, b in got["buf"].items():   # BatchNorm running_mean / running_var / num_batches_tracked, frozen layers included: they stay in training mode
        assert torch.equal(b, ref["buf"][k]), f"buffer {k}"
    assert any(k.endswith("num_batches_tracked") and int(b) == 1 for k, b in got["buf"].items())
    assert len(got["out"]) == len(ref["out"]) and all(torch.equal(a, b) for a, b in zip(got["out"], ref["out"]))


CASES = [("yolov3", torch.float16, [10]), ("yolov3", torch.float32, [10]), ("yolov3-tiny", torch.float16, [5]), ("yolov3-spp", torch.float16, [10]),
         ("yolov3", torch.float16, [4, 4]), ("yolov3", torch.float16, [27, 27]), ("yolov3", torch.float32, [4, 4])]


@pytest.mark.parametrize("name,dtype,freeze", CASES, ids=[f"{n}-{str(d).split('.')[-1]}-{'_'.join(map(str, f))}" for n, d, f in CASES])
def test_frozen_step_matches_the_unfrozen_step(dev, name, dtype, freeze):
    """prefix freezes ([10]: the backbone of yolov3 / yolov3-spp, [5] of yolov3-tiny) and two that are no prefix: layer 4 alone (a backbone stage in the middle: every
    data gradient still runs) and layer 27 alone (the last neck block: its input still needs a gradient)"""
    from yolov3_amd import freeze_layers

    ref = unfrozen(name, dtype, dev)
    m = make(name, dev)
    frozen = freeze_layers(m, freeze)
    assert frozen and all(not dict(m.named_parameters())[k].requires_grad for k in frozen)
    got = snapshot(m, step(m, image(dev), dtype))
    check_against_unfrozen(m, got, ref)


class Counter:
    """counts the calls of ops' training wrappers (the engine reaches the library through them alone) while installed"""

    NAMES = ("conv2d_wgrad", "stem_bn_bwd_wgrad", "conv2d", "conv2d_dgrad_s2", "bn_act_bwd", "bn_act_bwd_reduce", "pack_filter_dgrad")

    def __init__(self):
        from yolov3_amd import ops

        self.ops, self.calls, self.saved = ops, {n: [] for n in self.NAMES}, {}

    def __enter__(self):
        for n in self.NAMES:
            raw = self.saved[n] = getattr(self.ops, n)

            def fn(*a, raw_=raw, n_=n, **kw):
                self.calls[n_].append(a)
                return raw_(*a, **kw)
            setattr(self.ops, n, fn)
        return self

    def __exit__(self, *exc):
        for n, raw in self.saved.items():
            setattr(self.ops, n, raw)

    def n(self, *names):
        return sum(len(self.calls[k]) for k in names)


def backward_counts(m, x, dtype):
    from yolov3_amd import engine

    m.zero_grad(set_to_none=True)
    with torch.autocast("cuda", dtype=dtype):
        raws = m(x)
    g = torch.Generator().manual_seed(23)
    gs = [(torch.randn(r.shape, generator=g) * 0.01).to(r.device, r.dtype) for r in raws]
    with Counter() as c:   # the backward alone (autograd's thread calls the same module attributes)
        torch.autograd.backward(list(raws), gs)
        torch.cuda.synchronize()
    plan = next(p for k, p in engine.plan_cache(m).plans.items() if k[0] == "train" and p.generation > 0 and p.live == tuple(q.requires_grad for q in m.parameters()))
    return c, plan


def test_backbone_freeze_skips_the_launches(dev):
    """yolov3 [10]: one filter-gradient call per live conv weight, fewer data-gradient launches than the unfrozen step, no BatchNorm backward below layer 10"""
    from yolov3_amd import freeze_layers
    from yolov3_amd.train_engine import ConvUnit

    x = image(dev)
    full, _ = backward_counts(make("yolov3", dev), x, torch.float16)
    m = make("yolov3", dev)
    freeze_layers(m, [10])
    c, plan = backward_counts(m, x, torch.float16)
    wgrads = ("conv2d_wgrad", "stem_bn_bwd_wgrad")
    dgrads = ("conv2d", "conv2d_dgrad_s2")   # (inside the backward every conv2d launch is a data gradient)
    conv_weights = [p for k, p in m.named_parameters() if p.dim() == 4]
    live = sum(1 for p in conv_weights if p.requires_grad)
    assert len(conv_weights) == 75 and live == 75 - 44
    assert full.n(*wgrads) == 75 and c.n(*wgrads) == live
    assert full.n(*dgrads) == 74 and c.n(*dgrads) == 74 - 44, (full.n(*dgrads), c.n(*dgrads))   # (layers 0 .. 9: 43 data gradients, and the first live unit's)
    assert c.n(*dgrads) < full.n(*dgrads)
    below = {id(u.u) for u in plan.units if isinstance(u, ConvUnit) and int(u.label[1:].split(".")[0]) < 10}
    assert len(below) == 44
    touched = {id(a[0]) for a in c.calls["bn_act_bwd"] + c.calls["bn_act_bwd_reduce"]} | {id(a[1]) for a in c.calls["stem_bn_bwd_wgrad"]}
    assert not (touched & below) and c.n("stem_bn_bwd_wgrad") == 0
    assert full.n("bn_act_bwd") + full.n("stem_bn_bwd_wgrad") == 72 and c.n("bn_act_bwd") == 72 - 44
    assert c.n("pack_filter_dgrad") == 0   # every data gradient that runs found its bank packed with the forward's


def test_thaw_after_a_frozen_step(dev):
    """one FusedSGD step with the backbone frozen, then every parameter live: the second step's gradients are those of a never-frozen model at the same weights; the
    frozen weights did not move.  Then the thawed backbone is trained by a fused step (a kernel torch's version counter does not see) and frozen again: the frozen
    plan's banks must not be the ones it packed three steps ago."""
    from yolov3_amd import FusedSGD, freeze_layers, smart_param_groups

    x, dtype = image(dev), torch.float16
    m = make("yolov3", dev)
    frozen = set(freeze_layers(m, [10]))
    opt = FusedSGD(smart_param_groups(m, 0.01, 5e-4), momentum=0.937, nesterov=True)
    assert sum(len(g["params"]) for g in opt.param_groups) == sum(1 for p in m.parameters() if p.requires_grad)
    step(m, x, dtype)
    opt.step(grad_scale=1.0)
    torch.cuda.synchronize()
    sd0 = seeded_sd("yolov3")
    moved = 0
    for k, p in m.named_parameters():
        if k in frozen:
            assert torch.equal(p.detach().cpu(), sd0[k]), f"frozen {k} moved"
        else:
            moved += int(not torch.equal(p.detach().cpu(), sd0[k]))
    assert moved > 0
    assert freeze_layers(m, [0]) == []
    sd1 = {k: v.detach().clone() for k, v in m.state_dict().items()}
    outs = step(m, x, dtype)
    never = make("yolov3", dev, sd1)
    outs_n = step(never, x, dtype)
    assert all(torch.equal(a, b) for a, b in zip(outs, outs_n))
    grads_n = dict(never.named_parameters())
    for k, p in m.named_parameters():
        assert p.grad is not None and torch.equal(p.grad, grads_n[k].grad), f"gradient of {k} after the thaw"
    # train the backbone one step, freeze it again
    FusedSGD(smart_param_groups(m, 0.01, 5e-4), momentum=0.937, nesterov=True).step(grad_scale=1.0)
    torch.cuda.synchronize()
    freeze_layers(m, [10])
    sd2 = {k: v.detach().clone() for k, v in m.state_dict().items()}
    assert not torch.equal(sd2["model.1.conv.weight"], sd1["model.1.conv.weight"])
    outs = step(m, x, dtype)
    fresh = make("yolov3", dev, sd2)
    outs_f = step(fresh, x, dtype)
    assert all(torch.equal(a, b) for a, b in zip(outs, outs_f))


def test_frozen_banks_follow_load_state_dict(dev):
    """the frozen backbone's filter banks are packed once -- and again when load_state_dict writes other weights into the same tensors"""
    from yolov3_amd import engine, freeze_layers

    x, dtype = image(dev), torch.float16
    m = make("yolov3-tiny", dev)
    freeze_layers(m, [5])
    first = step(m, x, dtype)
    jobs = next(iter(engine.plan_cache(m).plans.values())).pack_jobs
    plan = next(iter(engine.plan_cache(m).plans.values()))
    assert len(jobs.stale(plan.pack_select)) == sum(1 for _, always in plan.pack_select if always) < len(plan.pack_select)   # the frozen banks are current
    again = step(m, x, dtype)   # (BatchNorm in training mode normalises with batch statistics: the same batch gives the same output)
    assert all(torch.equal(a, b) for a, b in zip(first, again))
    sd = {k: v.clone() for k, v in seeded_sd("yolov3-tiny").items()}
    g = torch.Generator().manual_seed(77)
    for k in sd:
        if k.endswith("conv.weight") and int(k.split(".")[1]) < 5:
            sd[k] = sd[k] + 0.05 * torch.randn(sd[k].shape, generator=g)
    m.load_state_dict(sd)
    assert all(not p.requires_grad for k, p in m.named_parameters() if int(k.split(".")[1]) < 5)
    assert len(jobs.stale(plan.pack_select)) > sum(1 for _, always in plan.pack_select if always)
    got = step(m, x, dtype)
    fresh = make("yolov3-tiny", dev, sd)
    want = step(fresh, x, dtype)
    assert not all(torch.equal(a, b) for a, b in zip(got, first))
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    for k, p in fresh.named_parameters():   # (and the live layers' gradients through the re-packed frozen banks)
        q = dict(m.named_parameters())[k]
        assert (q.grad is None) == (not q.requires_grad) and (q.grad is None or torch.equal(q.grad, p.grad)), k


def test_grad_buckets_see_live_gradients_only(dev):
    """one rank, forced through the bucket / side-stream / collective machinery as the existing one-rank test does: with the backbone frozen the bytes handed to the
    exchange are 4 x the live parameter count, and the (identity) average leaves the gradients those of the run without buckets"""
    import torch.distributed as dist

    from yolov3_amd import freeze_layers, parallel

    x, dtype = image(dev), torch.float16
    m = make("yolov3", dev)
    freeze_layers(m, [10])
    step(m, x, dtype)
    base = {k: (None if p.grad is None else p.grad.clone()) for k, p in m.named_parameters()}
    live = sum(p.numel() for p in m.parameters() if p.requires_grad)
    try:
        parallel.init("nccl", force=True)
        assert dist.is_initialized() and dist.get_world_size() == 1
        gb = parallel.GradBuckets(bucket_bytes=8 << 20, force=True)
        handed, reduced = [], []
        add, red = gb.add, gb._reduce
        gb.add = lambda key, grad: (handed.append((key, grad.numel() * grad.element_size())), add(key, grad))[1]
        gb._reduce = lambda flat: (reduced.append(flat._base is not None), red(flat))[1]
        m.grad_sync = gb
        step(m, x, dtype)
        assert sum(b for _, b in handed) == 4 * live
        assert all(k.requires_grad for k, _ in handed) and len(handed) == sum(1 for p in m.parameters() if p.requires_grad)
        assert len(reduced) >= 2 and all(reduced), "buckets are contiguous ranges of the (smaller) gradient arena"
        for k, p in m.named_parameters():
            assert (p.grad is None) == (base[k] is None) and (p.grad is None or torch.equal(p.grad, base[k])), k
    finally:
        m.grad_sync = None
        if dist.is_initialized():
            dist.destroy_process_group()
