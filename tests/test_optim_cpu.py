"""CPU tests of the fused Adam / AdamW / RMSProp surface (csrc/optim.hip, yolov3_amd.optim): the C ABI's declarations and argument validation without a GPU,
smart_optimizer, the unsupported flags, and the torch-format state dicts."""
import re
import subprocess
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
NEW_SYMBOLS = ["y3_optim_tensor_record_bytes", "y3_adam_step", "y3_rmsprop_step"]
TORCH = {"SGD": torch.optim.SGD, "Adam": torch.optim.Adam, "AdamW": torch.optim.AdamW, "RMSProp": torch.optim.RMSprop}


@pytest.fixture(scope="module")
def lib():
    from yolov3_amd import _lib, build

    build.build(verbose=False)
    return _lib.lib()


@pytest.fixture(scope="module")
def model():
    from yolov3_amd import DetectionModel

    return DetectionModel("yolov3-tiny.yaml")


def test_new_symbols_are_declared_bound_and_exported_at_abi_5(lib):
    from yolov3_amd import _lib

    header = (ROOT / "include" / "yolov3_hip.h").read_text()
    declared = set(re.findall(r"\b(y3_[a-z0-9_]+)\s*\(", header))
    assert set(NEW_SYMBOLS) <= declared and set(NEW_SYMBOLS) <= set(_lib.exported_symbols())
    assert "#define Y3_ABI_VERSION 6" in re.sub(r"[ \t]+", " ", header) and lib.y3_abi_version() == 6 == _lib.ABI_VERSION
    dynamic = subprocess.run(["nm", "-D", "--defined-only", str(_lib.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    assert all(re.search(rf"\bT {s}\b", dynamic) for s in NEW_SYMBOLS)
    assert lib.y3_optim_tensor_record_bytes() == 96 and lib.y3_sgd_tensor_record_bytes() == 56


def test_new_exports_reject_bad_arguments_without_a_gpu(lib):
    P = 1 << 20   # a fake, aligned device address: validation never dereferences it

    def fails(status, *needles):
        msg = lib.y3_last_error()
        assert status != 0 and all(msg.startswith(needles[0]) and n in msg for n in needles), (status, msg)

    #                 table n  chunks inv  scale max  dec  ema  step scratch found stream
    fails(lib.y3_adam_step(None, 3, 5, 1.0, None, 10.0, 0, 0.0, P, P, P, None), b"y3_adam_step", b"null tensor table")
    fails(lib.y3_adam_step(P, 0, 5, 1.0, None, 10.0, 0, 0.0, P, P, P, None), b"y3_adam_step", b"positive")
    fails(lib.y3_adam_step(P, 3, -1, 1.0, None, 10.0, 1, 0.0, P, P, P, None), b"y3_adam_step", b"positive")
    fails(lib.y3_adam_step(P, 3, 5, 1.0, P, 10.0, 1, 0.0, None, P, P, None), b"y3_adam_step", b"null step counter")
    fails(lib.y3_adam_step(P, 3, 5, 1.0, None, 10.0, 0, 0.0, P, None, P, None), b"y3_adam_step", b"scratch")
    fails(lib.y3_adam_step(P, 3, 5, 1.0, None, 10.0, 0, 0.0, P, P, None, None), b"y3_adam_step", b"found_inf")
    fails(lib.y3_rmsprop_step(None, 3, 5, 1.0, None, 10.0, 0.0, P, P, P, None), b"y3_rmsprop_step", b"null tensor table")
    fails(lib.y3_rmsprop_step(P, -2, 5, 1.0, None, 10.0, 0.0, P, P, P, None), b"y3_rmsprop_step", b"positive")
    fails(lib.y3_rmsprop_step(P, 3, 0, 1.0, None, 10.0, 0.0, P, P, P, None), b"y3_rmsprop_step", b"positive")
    fails(lib.y3_rmsprop_step(P, 3, 5, 1.0, P, 10.0, 0.0, None, P, P, None), b"y3_rmsprop_step", b"null step counter")
    fails(lib.y3_rmsprop_step(P, 3, 5, 1.0, None, 10.0, 0.0, P, None, None, None), b"y3_rmsprop_step", b"scratch")


def test_public_names():
    import yolov3_amd
    from yolov3_amd import FusedAdam, FusedAdamW, FusedRMSProp, optim, smart_optimizer

    assert (optim.FusedAdam, optim.FusedAdamW, optim.FusedRMSProp, optim.smart_optimizer) == (FusedAdam, FusedAdamW, FusedRMSProp, smart_optimizer)
    assert issubclass(FusedAdamW, FusedAdam) and callable(yolov3_amd.smart_optimizer)


@pytest.mark.parametrize("name,cls", [("SGD", "FusedSGD"), ("Adam", "FusedAdam"), ("AdamW", "FusedAdamW"), ("RMSProp", "FusedRMSProp")])
def test_smart_optimizer(model, name, cls):
    from yolov3_amd import optim

    opt = optim.smart_optimizer(model, name, lr=0.003, momentum=0.85, decay=2e-4)
    assert type(opt) is getattr(optim, cls)
    want = optim.smart_param_groups(model, 0.003, 2e-4)
    assert [len(g["params"]) for g in opt.param_groups] == [len(g["params"]) for g in want] and all(len(g["params"]) > 0 for g in want)
    assert all(a is b for g, h in zip(opt.param_groups, want) for a, b in zip(g["params"], h["params"]))
    assert [g["weight_decay"] for g in opt.param_groups] == [0.0, 2e-4, 0.0] and all(g["lr"] == 0.003 for g in opt.param_groups)
    if name == "SGD":
        assert opt.momentum == 0.85 and opt.nesterov is True
    elif name == "RMSProp":
        assert all(g["momentum"] == 0.85 and g["alpha"] == 0.99 and g["eps"] == 1e-8 for g in opt.param_groups)
    else:
        assert all(g["betas"] == (0.85, 0.999) and g["betas"][0] == 0.85 and g["eps"] == 1e-8 for g in opt.param_groups)


def test_smart_optimizer_defaults_and_unknown_name(model):
    from yolov3_amd import FusedAdam, smart_optimizer

    opt = smart_optimizer(model)
    assert type(opt) is FusedAdam and [(g["lr"], g["weight_decay"], g["betas"]) for g in opt.param_groups] == [(0.001, 0.0, (0.9, 0.999)), (0.001, 1e-5, (0.9, 0.999)),
                                                                                                               (0.001, 0.0, (0.9, 0.999))]
    with pytest.raises(NotImplementedError) as e:
        smart_optimizer(model, "Lion")
    assert str(e.value) == "Optimizer Lion not implemented."


def test_constructor_defaults_are_torchs():
    from yolov3_amd import FusedAdam, FusedAdamW, FusedRMSProp

    p = [torch.nn.Parameter(torch.zeros(3))]
    for ours, theirs in ((FusedAdam, torch.optim.Adam), (FusedAdamW, torch.optim.AdamW), (FusedRMSProp, torch.optim.RMSprop)):
        g, h = ours(p).param_groups[0], theirs(p).param_groups[0]
        assert all(g[k] == h[k] for k in g if k != "params"), (ours.__name__, g, h)
        assert {"lr", "eps", "weight_decay"} < set(g)


def test_unsupported_flags_raise():
    from yolov3_amd import FusedAdam, FusedAdamW, FusedRMSProp

    p = [torch.nn.Parameter(torch.zeros(3))]
    for cls, flag in ((FusedAdam, "amsgrad"), (FusedAdam, "maximize"), (FusedAdamW, "amsgrad"), (FusedAdamW, "maximize"), (FusedRMSProp, "centered"), (FusedRMSProp, "maximize")):
        with pytest.raises(ValueError, match=flag):
            cls(p, **{flag: True})
    sd = torch.optim.Adam(p, amsgrad=True).state_dict()
    with pytest.raises(ValueError, match="amsgrad"):
        FusedAdam(p).load_state_dict(sd)


@pytest.mark.parametrize("name", list(TORCH))
def test_fresh_state_dict_has_torchs_structure(model, name):
    from yolov3_amd import smart_optimizer, smart_param_groups

    opt = smart_optimizer(model, name, lr=0.004, momentum=0.8, decay=3e-4)
    sd = opt.state_dict()
    assert set(sd) == {"state", "param_groups"} and sd["state"] == {}
    n = sum(len(g["params"]) for g in opt.param_groups)
    assert [i for g in sd["param_groups"] for i in g["params"]] == list(range(n))
    kw = {"momentum": 0.1, "nesterov": True} if name == "SGD" else {}
    theirs = TORCH[name]([{"params": g["params"]} for g in smart_param_groups(model, 1.0, 0.5)], lr=1.0, **kw)
    assert set(sd["param_groups"][0]) == set(theirs.state_dict()["param_groups"][0])   # torch's keys, no more and no less
    theirs.load_state_dict(sd)
    assert [(g["lr"], g["weight_decay"]) for g in theirs.param_groups] == [(0.004, 0.0), (0.004, 3e-4), (0.004, 0.0)]
    if name in ("Adam", "AdamW"):
        assert all(g["betas"] == (0.8, 0.999) and g["decoupled_weight_decay"] is (name == "AdamW") for g in theirs.param_groups)
    else:
        assert all(g["momentum"] == 0.8 for g in theirs.param_groups)


@pytest.mark.parametrize("name", list(TORCH))
def test_torch_checkpoint_loads_and_comes_back(name):
    """a stepped torch optimizer's state dict loads (state on the parameters' device, hyper-parameters taken over) and state_dict() gives it back unchanged"""
    from yolov3_amd import optim

    ps = [torch.nn.Parameter(torch.randn(5)), torch.nn.Parameter(torch.randn(2, 3))]
    kw = {"momentum": 0.7, "nesterov": True} if name == "SGD" else {"momentum": 0.7} if name == "RMSProp" else {}
    theirs = TORCH[name](ps, lr=0.02, weight_decay=0.1, **kw)
    for _ in range(2):
        for p in ps:
            p.grad = torch.randn_like(p)
        theirs.step()
    ours = getattr(optim, {"SGD": "FusedSGD", "Adam": "FusedAdam", "AdamW": "FusedAdamW", "RMSProp": "FusedRMSProp"}[name])(ps)
    want = theirs.state_dict()
    ours.load_state_dict(want)
    got = ours.state_dict()
    assert got["param_groups"] == want["param_groups"] and set(got["state"]) == set(want["state"])
    for i, st in want["state"].items():
        assert set(got["state"][i]) == set(st)
        for k, v in st.items():
            assert torch.equal(got["state"][i][k], v) and got["state"][i][k].dtype == v.dtype, (i, k)
    if name == "SGD":
        assert ours.momentum == 0.7 and ours._steps > 0   # the next step is not a first step
    if name != "SGD":   # the fused step keeps ONE counter
        want["state"][1]["step"] = torch.tensor(9.0)
        with pytest.raises(ValueError, match="step"):
            ours.load_state_dict(want)


@pytest.mark.parametrize("cls", ["FusedAdam", "FusedAdamW", "FusedRMSProp"])
def test_step_on_cpu_parameters_raises(cls):
    from yolov3_amd import optim

    p = torch.nn.Parameter(torch.zeros(4))
    p.grad = torch.ones(4)
    with pytest.raises(RuntimeError, match="no CPU / PyTorch fallback"):
        getattr(optim, cls)([p]).step()
    assert torch.equal(p.detach(), torch.zeros(4))


# ------------------------------------------------------------------------------------------------ FusedSGD: momentum and nesterov live in the groups
def test_sgd_and_rmsprop_groups_carry_momentum_adam_groups_do_not(model):
    """the reference's warmup (train.py:383-391) writes ``x["momentum"]`` only ``if "momentum" in x``: true for SGD and RMSProp, false for Adam / AdamW, as with torch"""
    from yolov3_amd import FusedSGD, smart_optimizer, smart_param_groups

    for m in (0.85, 0.937):
        opt = smart_optimizer(model, "SGD", lr=0.01, momentum=m, decay=5e-4)
        assert len(opt.param_groups) == 3 and all(g["momentum"] == m and g["nesterov"] is True for g in opt.param_groups)
        assert opt.momentum == m and opt.nesterov is True
        plain = FusedSGD(smart_param_groups(model, 0.01, 5e-4), momentum=m, nesterov=False)
        assert all(g["momentum"] == m and g["nesterov"] is False for g in plain.param_groups) and plain.nesterov is False
    flat = FusedSGD([torch.nn.Parameter(torch.zeros(3))], momentum=0.6)   # a bare parameter list: one group
    assert [(g["momentum"], g["nesterov"]) for g in flat.param_groups] == [(0.6, True)]
    own = FusedSGD([{"params": [torch.nn.Parameter(torch.zeros(3))], "momentum": 0.5}], momentum=0.9)   # a group's own key wins, as in torch
    assert own.param_groups[0]["momentum"] == 0.5 and own.momentum == 0.5
    assert all("momentum" in g for g in smart_optimizer(model, "RMSProp", momentum=0.85).param_groups)
    for name in ("Adam", "AdamW"):
        theirs = TORCH[name]([torch.nn.Parameter(torch.zeros(3))])
        assert all("momentum" not in g and "betas" in g for g in smart_optimizer(model, name, momentum=0.85).param_groups) and "momentum" not in theirs.param_groups[0]
    assert "momentum" in torch.optim.SGD([torch.nn.Parameter(torch.zeros(3))], lr=0.1).param_groups[0]


def test_sgd_state_dict_follows_the_groups_momentum():
    """what a warmup wrote into the groups is what state_dict() reports (and torch.optim.SGD takes over); load_state_dict writes the loaded momentum into the groups"""
    from yolov3_amd import FusedSGD

    ps = [torch.nn.Parameter(torch.randn(5)), torch.nn.Parameter(torch.randn(2, 3))]
    groups = lambda: [{"params": [ps[0]], "weight_decay": 0.0}, {"params": [ps[1]], "weight_decay": 5e-4}]
    ours = FusedSGD(groups(), lr=0.01, momentum=0.937, nesterov=True)
    for g in ours.param_groups:
        g["momentum"] = 0.8685   # the reference's warmup, half way
    sd = ours.state_dict()
    assert [g["momentum"] for g in sd["param_groups"]] == [0.8685, 0.8685] and all(g["nesterov"] is True for g in sd["param_groups"]) and ours.momentum == 0.8685
    theirs = torch.optim.SGD(groups(), lr=1.0, momentum=0.1, nesterov=True)
    assert set(sd["param_groups"][0]) == set(theirs.state_dict()["param_groups"][0])
    theirs.load_state_dict(sd)
    assert [g["momentum"] for g in theirs.param_groups] == [0.8685, 0.8685]
    ours.momentum = 0.7   # the attribute is a property over the groups
    assert [g["momentum"] for g in ours.param_groups] == [0.7, 0.7]
    fresh = FusedSGD(groups(), lr=0.5, momentum=0.1, nesterov=False)
    fresh.load_state_dict(sd)
    assert [(g["momentum"], g["nesterov"], g["lr"]) for g in fresh.param_groups] == [(0.8685, True, 0.01)] * 2 and fresh.momentum == 0.8685 and fresh.nesterov is True
    sd["param_groups"][1]["momentum"] = 0.5
    with pytest.raises(ValueError, match="keeps one momentum for all groups"):
        fresh.load_state_dict(sd)
    assert [g["momentum"] for g in fresh.param_groups] == [0.8685, 0.8685]   # a refused checkpoint changes nothing


def test_sgd_step_with_differing_momenta_raises_before_any_launch():
    """CPU parameters with gradients: the agreement check comes first (ValueError), not the device check (RuntimeError: no CPU fallback), and nothing moved"""
    from yolov3_amd import FusedSGD

    ps = [torch.nn.Parameter(torch.zeros(4)), torch.nn.Parameter(torch.zeros(3))]
    for p in ps:
        p.grad = torch.ones_like(p)
    opt = FusedSGD([{"params": [ps[0]]}, {"params": [ps[1]]}], lr=0.1, momentum=0.9)
    opt.param_groups[1]["momentum"] = 0.8
    with pytest.raises(ValueError, match="keeps one momentum for all groups"):
        opt.step()
    with pytest.raises(ValueError, match="keeps one momentum for all groups"):
        opt.momentum
    assert all(torch.equal(p.detach(), torch.zeros_like(p)) for p in ps) and opt.state == {} and opt._steps == 0
    opt.param_groups[1]["momentum"] = 0.9   # in agreement again: the next refusal is the device's
    with pytest.raises(RuntimeError, match="no CPU / PyTorch fallback"):
        opt.step()


def test_ema_update_counted_is_declared_bound_exported_and_rejects_bad_arguments(lib):
    """the update behind a fused step (ModelEMA.after_step): count and decay on the device, nothing written after a skipped step"""
    from yolov3_amd import _lib

    header = (ROOT / "include" / "yolov3_hip.h").read_text()
    assert re.search(r"\by3_ema_update_counted\s*\(", header) and "y3_ema_update_counted" in _lib.exported_symbols()
    P = 1 << 20   # a fake, aligned device address: validation never dereferences it

    def fails(status, needle):
        msg = lib.y3_last_error()
        assert status != 0 and msg.startswith(b"y3_ema_update_counted") and needle in msg, (status, msg)

    fails(lib.y3_ema_update_counted(None, 3, 5, P, P, None), b"null tensor table")
    fails(lib.y3_ema_update_counted(P, 0, 5, P, P, None), b"positive")
    fails(lib.y3_ema_update_counted(P, 3, -1, P, None, None), b"positive")
    fails(lib.y3_ema_update_counted(P, 3, 5, None, P, None), b"null ema state")


def test_model_ema_updates_is_a_host_count_until_a_fused_step(model):
    from yolov3_amd import ModelEMA

    ema = ModelEMA(model, decay=0.99, tau=100, updates=7)
    assert ema.updates == 7 and ema._state is None
    d = ema.next_decay()
    assert ema.updates == 8 and d == pytest.approx(0.99 * (1 - torch.exp(torch.tensor(-8 / 100.0)).item()))
    ema.updates = 41
    assert ema.updates == 41 and ema._state is None
