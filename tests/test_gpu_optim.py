"""FusedAdam / FusedAdamW / FusedRMSProp (csrc/optim.hip: moment_update_kernel behind the two passes of the SGD step) on the MI355X against torch.optim's single-tensor
CPU algorithms on fp32 copies with the same gradient sequence, and the torch-format state dicts of all four fused optimizers.

The tensors are the smallest at which the kernel can still go wrong: numel 1, 3 and 255, a conv weight, 2 * 16384 + 5 elements (three blocks, a tail of one element
behind the last float4), one parameter at element offset 1 of a larger buffer (4-byte but not 16-byte aligned), and the gradients as views into one flat arena at odd
element offsets -- which sends every tensor down the scalar path, so every sequence also runs with separately allocated (16-byte aligned) gradients: the float4 path."""
import math
from pathlib import Path

import pytest
import torch
import yaml

from oracle import yolo_oracle as yo

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
CHUNK = 16384
SHAPES = [(1,), (3,), (255,), (64, 32, 3, 3), (2 * CHUNK + 5,), (1003,)]   # the last one is the misaligned view
GROUP_OF = [0, 1, 0, 1, 1, 0]
GROUP_HP = [dict(lr=2e-3, weight_decay=0.0, eps=1e-8), dict(lr=5e-3, weight_decay=5e-2, eps=1e-6)]
STEPS, SCALE, MAX_NORM = 5, 1024.0, 10.0
G_STD = 0.02          # gradient norm 0.02 * sqrt(52467) = 4.6 < MAX_NORM; step 1 is 30 times that
RTOL, ATOL = 1e-5, 1e-6

KINDS = {
    "Adam": ("FusedAdam", torch.optim.Adam, dict(betas=(0.9, 0.999))),
    "AdamW": ("FusedAdamW", torch.optim.AdamW, dict(betas=(0.8, 0.99))),
    "RMSProp": ("FusedRMSProp", torch.optim.RMSprop, dict(alpha=0.99, momentum=0.0)),
    "RMSProp-momentum": ("FusedRMSProp", torch.optim.RMSprop, dict(alpha=0.95, momentum=0.9)),
    "SGD": ("FusedSGD", torch.optim.SGD, dict(momentum=0.9, nesterov=True)),
}
MOMENT_KINDS = ["Adam", "AdamW", "RMSProp", "RMSProp-momentum"]
STATE_KEYS = {"Adam": ("exp_avg", "exp_avg_sq"), "AdamW": ("exp_avg", "exp_avg_sq"), "RMSProp": ("square_avg",), "RMSProp-momentum": ("square_avg", "momentum_buffer"),
              "SGD": ("momentum_buffer",)}
SQUARED = ("exp_avg_sq", "square_avg")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


def initial_values():
    g = torch.Generator().manual_seed(0)
    return [torch.randn(s, generator=g) for s in SHAPES]


def gradients(step, inf_at=None):
    g = torch.Generator().manual_seed(100 + step)
    out = [torch.randn(s, generator=g) * G_STD * (30.0 if step == 1 else 1.0) for s in SHAPES]   # step 1 exceeds max_norm
    if step == inf_at:
        out[4].view(-1)[CHUNK + 7] = float("inf")
    return out


def groups(params, kind):
    hp = [dict(h) for h in GROUP_HP]
    if kind == "SGD":
        for h in hp:
            h.pop("eps")
    return [{"params": [p for p, gi in zip(params, GROUP_OF) if gi == k], **hp[k]} for k in range(2)]


def device_params(dev, values):
    ps = []
    for i, v in enumerate(values):
        if i == len(values) - 1:
            buf = torch.zeros(v.numel() + 1, device=dev)
            buf[1:].copy_(v.view(-1))
            p = torch.nn.Parameter(buf[1:].view(v.shape))
            assert p.data_ptr() % 16 == 4 and p.is_contiguous()
        else:
            p = torch.nn.Parameter(v.to(dev))
        ps.append(p)
    return ps


def attach_gradients(ps, dev, arena):
    """arena: every gradient a view at an odd element offset of one flat buffer; otherwise one allocation each (16-byte aligned)"""
    if not arena:
        for p in ps:
            p.grad = torch.zeros_like(p)
            assert p.grad.data_ptr() % 16 == 0
        return
    offs, o = [], 1
    for p in ps:
        offs.append(o)
        o += p.numel() + p.numel() % 2   # keeps every offset odd
    flat = torch.zeros(o, device=dev)
    for p, o in zip(ps, offs):
        p.grad = flat[o:o + p.numel()].view(p.shape)
        assert o % 2 == 1 and p.grad.data_ptr() % 16 != 0


class Holder(torch.nn.Module):
    def __init__(self, q):
        super().__init__()
        self.q = torch.nn.ParameterList(q)


def make_fused(kind, ps):
    from yolov3_amd import optim

    name, _, kw = KINDS[kind]
    return getattr(optim, name)(groups(ps, kind), **kw)


def make_torch(kind, ps):
    return KINDS[kind][1](groups(ps, kind), **KINDS[kind][2])


def lr_of_group1(step):
    return GROUP_HP[1]["lr"] * (1.0 - 0.15 * step)   # a scheduler rewriting group["lr"] between steps


def snapshot(kind, params, state_of, ema, norm):
    return {"p": [p.detach().cpu().clone() for p in params], "ema": [e.cpu().clone() for e in ema], "norm": norm,
            "state": [{k: state_of(p)[k].cpu().clone() for k in STATE_KEYS[kind]} for p in params]}


_TORCH: dict = {}


def torch_run(kind, inf_at=None, dtype=torch.float32):
    """the reference sequence on the CPU (clip_grad_norm_, torch.optim step, the EMA lerp); a step with an inf gradient is one torch's GradScaler would not make:
    no step(), no lerp, and ModelEMA's update count does not advance either (the fused path keeps it on the device).  Computed once per case and shared."""
    key = (kind, inf_at, dtype)
    if key in _TORCH:
        return _TORCH[key]
    ref = [torch.nn.Parameter(v.to(dtype)) for v in initial_values()]
    opt = make_torch(kind, ref)
    ema = [p.detach().clone() for p in ref]
    snaps, updates = [], 0
    for step in range(STEPS):
        opt.param_groups[1]["lr"] = lr_of_group1(step)
        for r, g in zip(ref, gradients(step, inf_at)):
            r.grad = g.to(dtype)
        norm = None
        if step != inf_at:
            updates += 1
            d = 0.9999 * (1 - math.exp(-updates / 2000))
            norm = float(torch.nn.utils.clip_grad_norm_(ref, max_norm=MAX_NORM))
            opt.step()
            for e, r in zip(ema, ref):
                e.mul_(d).add_(r.detach(), alpha=1 - d)
        snaps.append(snapshot(kind, ref, lambda p: opt.state[p], ema, norm))
    _TORCH[key] = snaps
    return snaps


def fused_run(kind, dev, arena, inf_at=None):
    from yolov3_amd.optim import ModelEMA

    ps = device_params(dev, initial_values())
    attach_gradients(ps, dev, arena)
    opt = make_fused(kind, ps)
    ema = ModelEMA(Holder(ps))
    snaps, counters = [], []
    for step in range(STEPS):
        opt.param_groups[1]["lr"] = lr_of_group1(step)
        for p, g in zip(ps, gradients(step, inf_at)):
            p.grad.copy_((g * SCALE).to(dev))
        opt.step(grad_scale=SCALE, max_norm=MAX_NORM, ema=ema)
        torch.cuda.synchronize()
        assert int(opt.found_inf.item()) == int(step == inf_at)
        snaps.append(snapshot(kind, ps, lambda p: opt.state[p], [ema.shadow[p] for p in ps], float(opt.last_norm.item())))
        counters.append(int(opt._step_dev.item()))
    assert ema.updates == STEPS - (inf_at is not None)   # a skipped step is no update of the average
    return snaps, counters


_WORST: dict = {}


def fp32_worst_error(kind, key, inf_at=None):
    """the fp32 CPU run's own worst absolute error in state buffer `key` against the same sequence in torch fp64 (same fp32 gradients and initial values), over
    all steps and tensors"""
    k_ = (kind, key, inf_at)
    if k_ not in _WORST:
        a32, a64 = torch_run(kind, inf_at), torch_run(kind, inf_at, torch.float64)
        _WORST[k_] = max(float((x["state"][i][key].double() - y["state"][i][key]).abs().max()) for x, y in zip(a32, a64) for i in range(len(SHAPES)))
    return _WORST[k_]


def check_step(kind, got, want, what, inf_at=None):
    if want["norm"] is not None:
        print(f"[{what}] norm {got['norm']:.7g} vs {want['norm']:.7g}")
        assert abs(got["norm"] - want["norm"]) / want["norm"] < 1e-5, what
    for i in range(len(SHAPES)):
        torch.testing.assert_close(got["p"][i], want["p"][i], rtol=RTOL, atol=ATOL, msg=lambda m: f"{what} param {i}: {m}")
        torch.testing.assert_close(got["ema"][i], want["ema"][i], rtol=RTOL, atol=ATOL, msg=lambda m: f"{what} ema {i}: {m}")
        for k in STATE_KEYS[kind]:
            a, b = got["state"][i][k], want["state"][i][k]
            atol = ATOL
            if k == "momentum_buffer":   # RMSProp's buffer of g / (sqrt(s) + eps): see test_fused_step_vs_torch
                atol = max(ATOL, 4.0 * fp32_worst_error(kind, k, inf_at))
            torch.testing.assert_close(a, b, rtol=RTOL, atol=atol, msg=lambda m: f"{what} {k} {i}: {m}")
            if k in SQUARED:
                # the squared averages are ~1e-7 here, under the project's atol.  They are sums of positive terms, three fp32 roundings a step on top of the clip
                # coefficient's 1e-7: the same rtol holds with atol scaled to the buffer
                torch.testing.assert_close(a, b, rtol=RTOL, atol=ATOL * float(b.abs().max()), msg=lambda m: f"{what} {k} {i} (scaled atol): {m}")


@pytest.mark.parametrize("arena", [True, False], ids=["arena-odd-offsets", "aligned-grads"])
@pytest.mark.parametrize("kind", MOMENT_KINDS)
def test_fused_step_vs_torch(dev, kind, arena):
    """five steps: loss scale 1024, max_norm 10 with step 1 above it, EMA on, group 1's lr rewritten before every step; parameters, every state buffer, the EMA
    shadow and last_norm after every step, at the SGD test's tolerances (rtol 1e-5, atol 1e-6, norm 1e-5 relative).

    One buffer needs more, and gets a derived bound instead of a tuned one: RMSProp's momentum buffer accumulates g / (sqrt(s) + eps) with g = grad + wd * p, and where
    that sum cancels to ~1e-6 (below eps-scale) the quotient is ill-conditioned -- the last-bit rounding of wd * p (ATen's CPU add(alpha) fuses it, the kernel rounds
    twice) moves it by 1e-5 .. 1e-4.  The same sequence in torch fp64 (same fp32 gradients and initial values) shows the fp32 CPU run's OWN worst absolute error in
    that buffer: 1.03e-4; the test allows 4 x that = 4.12e-4 as atol (fp32_worst_error, computed at run time), rtol unchanged.  Every other buffer, the parameters and
    the EMA stay at the project's tolerances (the fp32 run's worst errors against fp64 there: exp_avg 1.2e-8, exp_avg_sq 1.0e-10, square_avg 2.1e-9)."""
    got, counters = fused_run(kind, dev, arena)
    want = torch_run(kind)
    assert counters == [1, 2, 3, 4, 5]
    for step in range(STEPS):
        check_step(kind, got[step], want[step], f"{kind} step {step}")
    moved = (got[-1]["p"][4] - initial_values()[4]).abs().max().item()
    assert moved > 1e-3, "the parameters did not move"


@pytest.mark.parametrize("kind", ["Adam", "RMSProp-momentum"])
def test_skipped_step(dev, kind):
    """an inf gradient at the third step: parameters, state and EMA stay bit for bit, the device step counter does not advance, and the two steps after it match a
    torch run that made no step() there (a wrong t shows in Adam's bias corrections)"""
    inf_at = 2
    got, counters = fused_run(kind, dev, True, inf_at=inf_at)
    want = torch_run(kind, inf_at=inf_at)
    assert counters == [1, 2, 2, 3, 4]
    for key in ("p", "ema"):
        assert all(torch.equal(a, b) for a, b in zip(got[inf_at][key], got[inf_at - 1][key])), key
    for a, b in zip(got[inf_at]["state"], got[inf_at - 1]["state"]):
        assert all(torch.equal(a[k], b[k]) for k in a)
    for step in range(STEPS):
        check_step(kind, got[step], want[step], f"{kind} step {step} (skip at {inf_at})", inf_at)


def test_grad_scaler_drives_fused_adam(dev):
    """optim.GradScaler (device scale) through growth and backoff against the same sequence with the scale applied by hand: powers of two, so bit for bit"""
    from yolov3_amd.optim import FusedAdam, GradScaler

    vals = initial_values()
    a, b = device_params(dev, vals), device_params(dev, vals)
    attach_gradients(a, dev, True)
    attach_gradients(b, dev, True)
    oa, ob = FusedAdam(groups(a, "Adam")), FusedAdam(groups(b, "Adam"))
    scaler = GradScaler(init_scale=2.0**10, growth_factor=2.0, backoff_factor=0.5, growth_interval=2)
    scaler._lazy(dev)
    by_hand = [1024.0, 1024.0, 2048.0, 1024.0, 1024.0, 2048.0, 1024.0]   # growth after two clean steps, backoff after the overflows at steps 2 and 5
    for step, s in enumerate(by_hand):
        g = gradients(step % STEPS, inf_at=step % STEPS if step in (2, 5) else None)
        for p, q, gi in zip(a, b, g):
            p.grad.copy_(gi.to(dev) * scaler._scale)
            q.grad.copy_((gi * s).to(dev))
        scaler.unscale_(oa)
        scaler.step(oa, max_norm=MAX_NORM)
        scaler.update()
        ob.step(grad_scale=s, max_norm=MAX_NORM)
    torch.cuda.synchronize()
    assert scaler.get_scale() == 1024.0 and int(oa._step_dev.item()) == int(ob._step_dev.item()) == 5
    for p, q in zip(a, b):
        assert torch.equal(p.detach(), q.detach())
        assert all(torch.equal(oa.state[p][k], ob.state[q][k]) for k in ("exp_avg", "exp_avg_sq"))


def _plain_steps(opt, params, steps, dev=None):
    for step in steps:
        for p, g in zip(params, gradients(step)):
            if dev is None:
                p.grad = g.clone()
            else:
                p.grad.copy_(g.to(dev))
        opt.step()
    if dev is not None:
        torch.cuda.synchronize()


def _compare_after_interchange(kind, ps, fused, ref, topt, what):
    for i, (p, r) in enumerate(zip(ps, ref)):
        torch.testing.assert_close(p.detach().cpu(), r.detach(), rtol=RTOL, atol=ATOL, msg=lambda m: f"{what} param {i}: {m}")
        for k in STATE_KEYS[kind]:
            st = fused.state[p]
            torch.testing.assert_close((st if kind == "SGD" else st[k]).cpu(), topt.state[r][k], rtol=RTOL, atol=ATOL, msg=lambda m: f"{what} {k} {i}: {m}")


@pytest.mark.parametrize("kind", ["SGD"] + MOMENT_KINDS)
def test_state_dict_interchange(dev, kind):
    """three steps in torch, load_state_dict here, three more on both sides; then the reverse.  For FusedSGD the step after loading is no first step (a first step
    would store buf = g instead of mu * buf + g)."""
    # torch -> fused
    ref = [torch.nn.Parameter(v) for v in initial_values()]
    topt = make_torch(kind, ref)
    _plain_steps(topt, ref, range(3))
    ps = device_params(dev, [r.detach().clone() for r in ref])
    attach_gradients(ps, dev, True)
    fused = make_fused(kind, ps)
    for g in fused.param_groups:
        g["lr"] = 123.0   # overwritten by the checkpoint
    fused.load_state_dict(topt.state_dict())
    assert [g["lr"] for g in fused.param_groups] == [h["lr"] for h in GROUP_HP]
    if kind == "SGD":
        assert fused._steps > 0
    _plain_steps(topt, ref, range(3, 6))
    _plain_steps(fused, ps, range(3, 6), dev)
    _compare_after_interchange(kind, ps, fused, ref, topt, f"{kind} torch->fused")
    sd = fused.state_dict()
    assert all(t.device == ps[0].device for st in sd["state"].values() for k, t in st.items() if k != "step")
    if kind != "SGD":
        assert all(float(st["step"]) == 6.0 for st in sd["state"].values())
    # fused -> torch (from the state reached above: six steps)
    ref2 = [torch.nn.Parameter(p.detach().cpu().clone()) for p in ps]
    topt2 = make_torch(kind, ref2)
    topt2.load_state_dict(sd)
    _plain_steps(topt2, ref2, range(6, 9))
    _plain_steps(fused, ps, range(6, 9), dev)
    _compare_after_interchange(kind, ps, fused, ref2, topt2, f"{kind} fused->torch")
    if kind != "SGD":
        assert all(float(topt2.state[r]["step"]) == 9.0 for r in ref2) and int(fused._step_dev.item()) == 9


def test_load_state_dict_rejects_differing_steps(dev):
    ref = [torch.nn.Parameter(v) for v in initial_values()]
    topt = make_torch("Adam", ref)
    _plain_steps(topt, ref, range(2))
    sd = topt.state_dict()
    sd["state"][0]["step"] = torch.tensor(7.0)
    with pytest.raises(ValueError, match="step"):
        make_fused("Adam", device_params(dev, initial_values())).load_state_dict(sd)


@pytest.mark.parametrize("kind", ["Adam", "RMSProp-momentum"])
def test_deterministic(dev, kind):
    """the same five steps twice: bit-identical parameters, state, EMA and norm"""
    a, _ = fused_run(kind, dev, False)
    b, _ = fused_run(kind, dev, False)
    for x, y in zip(a, b):
        assert x["norm"] == y["norm"]
        assert all(torch.equal(p, q) for p, q in zip(x["p"], y["p"])) and all(torch.equal(p, q) for p, q in zip(x["ema"], y["ema"]))
        assert all(torch.equal(s[k], t[k]) for s, t in zip(x["state"], y["state"]) for k in s)


def test_whole_model_adamw_step(dev):
    """one smart_optimizer(model, "AdamW") step on yolov3-tiny at 64 x 64, batch 2, through the training engine and ComputeLoss, layers 0-1 frozen: every parameter
    with a gradient moved and stayed finite, the frozen ones did not move and have no state"""
    from yolov3_amd import ComputeLoss, DetectionModel, FusedAdamW, freeze_layers, smart_optimizer

    nc, hw, bs = 80, 64, 2
    d = yaml.safe_load(open(ROOT / "yolov3_amd" / "cfg" / "yolov3-tiny.yaml"))
    layers, _, anchors, nc_v = yo.parse_cfg(d, 3, nc)
    sd0 = yo.seeded_state_dict(layers, nc_v, anchors, yo.model_strides(layers), seed=11)
    m = DetectionModel("yolov3-tiny.yaml", nc=nc)
    m.load_state_dict(sd0)
    m = m.to(dev).train()
    nl = m.model[-1].nl
    m.hyp = dict(box=0.05 * 3 / nl, cls=0.5 * nc / 80 * 3 / nl, cls_pw=1.0, obj=(hw / 640) ** 2 * 3 / nl, obj_pw=1.0, anchor_t=4.0, fl_gamma=0.0, label_smoothing=0.0)
    frozen = set(freeze_layers(m, [2]))
    assert frozen
    opt = smart_optimizer(m, "AdamW", lr=1e-3, momentum=0.9, decay=1e-2)
    assert isinstance(opt, FusedAdamW)
    crit = ComputeLoss(m)
    x = torch.rand(bs, 3, hw, hw, generator=torch.Generator().manual_seed(5)).to(dev)
    tg = yo.synth_targets(bs, nc, seed=1).to(dev)
    loss, _ = crit(m(x), tg)
    loss.backward()
    opt.step(grad_scale=1.0, max_norm=10.0)
    torch.cuda.synchronize()
    assert int(opt.found_inf.item()) == 0 and math.isfinite(opt.last_norm.item()) and int(opt._step_dev.item()) == 1
    live = 0
    for k, p in m.named_parameters():
        if k in frozen:
            assert p.grad is None and p not in opt.state and torch.equal(p.detach().cpu(), sd0[k]), f"frozen {k}"
        else:
            live += 1
            assert p.grad is not None and p in opt.state, k
            assert bool(torch.isfinite(p).all()) and not torch.equal(p.detach().cpu(), sd0[k]), f"{k} did not move"
    assert live > 0 and len(opt.state) == live
