"""CPU tests of the EMA-model / checkpoint surface: the two exports behind it (y3_ema_update in csrc/optim.hip, y3_fold_pack_jobs in csrc/filter_bank.hip) are declared, bound,
exported and validate their arguments without a GPU; ModelEMA is backed by a real module; save_checkpoint / smart_resume / strip_optimizer / attempt_load round-trip
the reference's checkpoint dict on CPU objects (no launch is needed for any of it)."""
import re
import subprocess
import sys
from copy import deepcopy
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
NEW_SYMBOLS = ["y3_ema_update", "y3_fold_pack_jobs"]


@pytest.fixture(scope="module")
def lib():
    from yolov3_amd import _lib, build

    build.build(verbose=False)
    return _lib.lib()


@pytest.fixture(scope="module")
def model():
    from yolov3_amd import DetectionModel

    torch.manual_seed(3)
    m = DetectionModel("yolov3-tiny.yaml", nc=3)
    for mod in m.modules():
        if isinstance(mod, torch.nn.BatchNorm2d):
            mod.running_mean.normal_(0, 0.1)
            mod.running_var.uniform_(0.5, 1.5)
    return m


def test_new_symbols_are_declared_bound_and_exported_at_abi_5(lib):
    from yolov3_amd import _lib

    header = (ROOT / "include" / "yolov3_hip.h").read_text()
    declared = set(re.findall(r"\b(y3_[a-z0-9_]+)\s*\(", header))
    assert set(NEW_SYMBOLS) <= declared and set(NEW_SYMBOLS) <= set(_lib.exported_symbols())
    assert "#define Y3_ABI_VERSION 6" in re.sub(r"[ \t]+", " ", header) and lib.y3_abi_version() == 6 == _lib.ABI_VERSION
    dynamic = subprocess.run(["nm", "-D", "--defined-only", str(_lib.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    assert all(re.search(rf"\bT {s}\b", dynamic) for s in NEW_SYMBOLS)
    assert "typedef struct y3_fold_pack_job" in header


def test_new_exports_reject_bad_arguments_without_a_gpu(lib):
    from yolov3_amd import _lib

    P = 1 << 20   # a fake, aligned device address: validation never dereferences it

    def fails(status, *needles):
        msg = lib.y3_last_error()
        assert status != 0 and all(msg.startswith(needles[0]) and n in msg for n in needles), (status, msg)

    #                      table n  chunks d   stream
    fails(lib.y3_ema_update(None, 3, 5, 0.5, None), b"y3_ema_update", b"null tensor table")
    fails(lib.y3_ema_update(P, 0, 5, 0.5, None), b"y3_ema_update", b"positive")
    fails(lib.y3_ema_update(P, -1, 5, 0.5, None), b"y3_ema_update", b"positive")
    fails(lib.y3_ema_update(P, 3, -4, 0.5, None), b"y3_ema_update", b"positive")
    fails(lib.y3_ema_update(P, 3, 5, 1.5, None), b"y3_ema_update", b"decay")
    fails(lib.y3_ema_update(P, 3, 5, float("nan"), None), b"y3_ema_update", b"decay")
    #                          table jobs blocks dtype      stream
    fails(lib.y3_fold_pack_jobs(None, 2, 7, _lib.Y3_F16, None), b"y3_fold_pack_jobs", b"null job table")
    fails(lib.y3_fold_pack_jobs(P, 0, 7, _lib.Y3_F16, None), b"y3_fold_pack_jobs", b"positive")
    fails(lib.y3_fold_pack_jobs(P, -3, 7, _lib.Y3_BF16, None), b"y3_fold_pack_jobs", b"positive")
    fails(lib.y3_fold_pack_jobs(P, 2, -1, _lib.Y3_F32, None), b"y3_fold_pack_jobs", b"positive")
    fails(lib.y3_fold_pack_jobs(P, 2, 1 << 31, _lib.Y3_F32, None), b"y3_fold_pack_jobs", b"fit a grid")
    fails(lib.y3_fold_pack_jobs(P, 2, 7, _lib.Y3_U8, None), b"y3_fold_pack_jobs", b"bad dtype")
    fails(lib.y3_fold_pack_jobs(P, 2, 7, 17, None), b"y3_fold_pack_jobs", b"bad dtype")


def test_public_names():
    import yolov3_amd
    from yolov3_amd import ModelEMA, compat, save_checkpoint, smart_resume, strip_optimizer

    assert (compat.save_checkpoint, compat.smart_resume, compat.strip_optimizer) == (save_checkpoint, smart_resume, strip_optimizer)
    assert all(callable(getattr(ModelEMA, n)) for n in ("update", "update_attr", "next_decay", "update_buffers", "update_rest"))
    assert yolov3_amd.DetectionModel.infer_dtype is None and yolov3_amd.DetectionModel.weights_epoch == 0
    from yolov3_amd import engine

    assert isinstance(engine.EVAL_PLAN_BUILDS, int) and callable(engine.FoldPackJobs)
    import inspect

    assert list(inspect.signature(smart_resume).parameters) == ["ckpt", "optimizer", "ema", "weights", "epochs", "resume"]
    assert list(inspect.signature(save_checkpoint).parameters)[:6] == ["path", "model", "ema", "optimizer", "epoch", "best_fitness"]
    assert {"half", "dtype"} <= set(inspect.signature(yolov3_amd.run_batches).parameters) and {"half", "dtype"} <= set(inspect.signature(yolov3_amd.detect_batches).parameters)


def test_model_ema_is_backed_by_a_module(model):
    from yolov3_amd import DetectionModel, ModelEMA

    m = deepcopy(model).train()
    ema = ModelEMA(m, decay=0.99, tau=100, updates=7)
    assert type(ema.ema) is DetectionModel and ema.ema is not m and not ema.ema.training and m.training
    assert all(not p.requires_grad for p in ema.ema.parameters()) and all(p.requires_grad for p in m.parameters())
    assert (ema.decay, ema.tau, ema.updates) == (0.99, 100, 7)
    # shadow / buffers: the training model's tensors -> the very parameters / float buffers of ema.ema (no second copy)
    mp, ep = dict(m.named_parameters()), dict(ema.ema.named_parameters())
    assert len(ema.shadow) == len(mp) and all(ema.shadow[mp[k]] is ep[k] for k in mp)
    mb, eb = dict(m.named_buffers()), dict(ema.ema.named_buffers())
    fl = [k for k, b in mb.items() if b.dtype.is_floating_point]
    assert len(ema.buffers) == len(fl) > 0 and all(ema.buffers[mb[k]] is eb[k] for k in fl)
    assert all(torch.equal(v, ema.ema.state_dict()[k]) and v.data_ptr() != ema.ema.state_dict()[k].data_ptr() for k, v in m.state_dict().items())
    assert ema.ema.stride.tolist() == m.stride.tolist()
    d = ema.next_decay()
    assert ema.updates == 8 and d == pytest.approx(0.99 * (1 - torch.exp(torch.tensor(-8 / 100.0)).item()))
    e0 = ema.ema.weights_epoch
    ema.touched()
    assert ema.ema.weights_epoch == e0 + 1 and m.weights_epoch == 0
    # a wrapped model is averaged without its wrapper, as upstream (de_parallel)
    wrapped = torch.nn.DataParallel(m)
    assert type(ModelEMA(wrapped).ema) is DetectionModel


def test_update_on_cpu_tensors_raises_and_changes_nothing(model):
    from yolov3_amd import ModelEMA

    m = deepcopy(model)
    ema = ModelEMA(m)
    before = {k: v.clone() for k, v in ema.ema.state_dict().items()}
    with pytest.raises(RuntimeError, match="no CPU / PyTorch fallback"):
        ema.update(m)
    assert all(torch.equal(v, before[k]) for k, v in ema.ema.state_dict().items())


def test_update_attr_follows_upstream_copy_attr(model):
    from yolov3_amd import ModelEMA

    m = deepcopy(model)
    ema = ModelEMA(m)
    m.nc, m.hyp, m.names, m.class_weights = 3, {"box": 0.05}, {0: "a", 1: "b", 2: "c"}, torch.tensor([1.0, 2.0, 3.0])
    m.process_group, m.other, m._private = "pg", 5, 6
    ema.update_attr(m, include=["yaml", "nc", "hyp", "names", "stride", "class_weights"])
    e = ema.ema
    assert e.nc == 3 and e.hyp is m.hyp and e.names is m.names and e.class_weights is m.class_weights and e.stride is m.stride
    assert not hasattr(e, "other") and not hasattr(e, "process_group") and not hasattr(e, "_private")
    ema.update_attr(m)   # everything that is neither private nor excluded
    assert e.other == 5 and not hasattr(e, "process_group") and not hasattr(e, "_private")


def _ckpt_objects(model):
    from yolov3_amd import FusedSGD, ModelEMA, smart_param_groups

    m = deepcopy(model)
    ema = ModelEMA(m, updates=41)
    with torch.no_grad():
        for p in ema.ema.parameters():   # an average that differs from the weights
            p.mul_(0.75)
    opt = FusedSGD(smart_param_groups(m, 0.01, 5e-4), momentum=0.9, nesterov=True)
    for g in opt.param_groups:
        for p in g["params"]:
            opt.state[p] = torch.full_like(p, 0.125)
    opt._steps = 1
    return m, ema, opt


def test_checkpoint_round_trip_on_cpu(model, tmp_path):
    from yolov3_amd import DetectionModel, FusedSGD, ModelEMA, attempt_load, compat, save_checkpoint, smart_param_groups, smart_resume, strip_optimizer

    m, ema, opt = _ckpt_objects(model)
    f = tmp_path / "last.pt"
    save_checkpoint(f, m, ema, opt, epoch=4, best_fitness=0.25, date="today")
    ck = compat.load_checkpoint(f)
    assert set(ck) == {"epoch", "best_fitness", "model", "ema", "updates", "optimizer", "date"}
    assert (ck["epoch"], ck["best_fitness"], ck["updates"], ck["date"]) == (4, 0.25, 41, "today")
    assert type(ck["model"]) is DetectionModel and type(ck["ema"]) is DetectionModel
    assert all(v.dtype == torch.float16 for md in (ck["model"], ck["ema"]) for v in md.state_dict().values() if v.is_floating_point())
    assert all(p.dtype == torch.float32 for p in m.parameters()) and all(p.dtype == torch.float32 for p in ema.ema.parameters())   # the masters were not touched
    assert all(torch.equal(v, ema.ema.state_dict()[k].half()) for k, v in ck["ema"].state_dict().items() if v.is_floating_point())
    assert not any(k.startswith("_plans") or "plan" in k for k in ck["ema"].__dict__)
    # attempt_load prefers the averaged model
    got = attempt_load(f, device="cpu", fuse=False)
    assert all(torch.equal(v, ema.ema.state_dict()[k].half().float()) for k, v in got.state_dict().items() if v.is_floating_point())
    # resume into fresh objects
    m2 = DetectionModel("yolov3-tiny.yaml", nc=3)
    ema2, opt2 = ModelEMA(m2), FusedSGD(smart_param_groups(m2, 0.1, 0.0), momentum=0.5, nesterov=False)
    e0 = ema2.ema.weights_epoch
    assert smart_resume(ck, opt2, ema2, weights="last.pt", epochs=300, resume=True) == (0.25, 5, 300)
    assert ema2.updates == 41 and ema2.ema.weights_epoch > e0
    assert all(torch.equal(v, ema.ema.state_dict()[k].half().float()) for k, v in ema2.ema.state_dict().items() if v.is_floating_point())
    assert all(p.dtype == torch.float32 and not p.requires_grad for p in ema2.ema.parameters())
    assert opt2.momentum == 0.9 and opt2.nesterov is True and [g["lr"] for g in opt2.param_groups] == [0.01] * 3
    assert all(torch.equal(opt2.state[p], torch.full_like(p, 0.125)) for g in opt2.param_groups for p in g["params"])
    assert smart_resume(ck, None, None, epochs=3, resume=False) == (0.0, 5, 7)   # fewer epochs than done: fine-tune that many more
    # strip
    s = tmp_path / "best.pt"
    x = strip_optimizer(f, s)
    y = compat.load_checkpoint(s)
    for d in (x, y):
        assert d["ema"] is None and d["optimizer"] is None and d["best_fitness"] is None and d["updates"] is None and d["epoch"] == -1
        assert all(p.dtype == torch.float16 and not p.requires_grad for p in d["model"].parameters())
    assert all(torch.equal(v, ck["ema"].state_dict()[k]) for k, v in y["model"].state_dict().items())
    assert s.stat().st_size < 0.6 * f.stat().st_size
    assert type(attempt_load(s, device="cpu")) is DetectionModel
    strip_optimizer(f)   # in place
    assert compat.load_checkpoint(f)["epoch"] == -1


def _run_py(code, cwd):
    return subprocess.check_output([sys.executable, "-c", code], cwd=cwd, text=True, stderr=subprocess.STDOUT)


def test_saved_checkpoint_loads_in_a_process_without_the_reference(model, tmp_path):
    from yolov3_amd import save_checkpoint

    m, ema, opt = _ckpt_objects(model)
    f = tmp_path / "last.pt"
    save_checkpoint(f, m, ema, opt, epoch=0)
    code = f"""
import sys, torch
sys.path.insert(0, {str(ROOT)!r})
from yolov3_amd import compat, DetectionModel
m = compat.attempt_load({str(f)!r}, device='cpu')
assert type(m) is DetectionModel and not any(k == 'models' or k.startswith('models.') for k in sys.modules)
ck = compat.load_checkpoint({str(f)!r})
assert ck['updates'] == 41 and type(ck['ema']) is DetectionModel
print('ok')
"""
    assert _run_py(code, tmp_path).strip().endswith("ok")


def test_saved_checkpoint_loads_inside_a_live_reference_process(model, tmp_path):
    """the scoped unpickler resolves this package's own class paths as usual while the REAL models.yolo / models.common are imported"""
    from oracle import ref_shim
    from yolov3_amd import save_checkpoint

    if not ref_shim.available():
        pytest.skip("reference tree not present on this box")
    m, ema, opt = _ckpt_objects(model)
    f = tmp_path / "last.pt"
    save_checkpoint(f, m, ema, opt, epoch=0)
    code = f"""
import sys, torch
sys.path.insert(0, {str(ROOT)!r})
from oracle import ref_shim
ns = ref_shim.load()
import models.yolo as real_yolo
from yolov3_amd import compat, DetectionModel
before = (sys.modules['models'], sys.modules['models.yolo'], sys.modules['models.common'])
m = compat.attempt_load({str(f)!r}, device='cpu')
assert type(m) is DetectionModel and type(m) is not real_yolo.DetectionModel
assert before == (sys.modules['models'], sys.modules['models.yolo'], sys.modules['models.common'])
print('ok')
"""
    assert _run_py(code, tmp_path).strip().endswith("ok")


def test_fold_pack_switch_and_job_bookkeeping(model, monkeypatch):
    """host side of FoldPackJobs without a launch: banks are sized like the per-layer path's, the switch is read per call"""
    from yolov3_amd import engine, ops

    monkeypatch.delenv("Y3_FOLD_PACK", raising=False)
    assert engine.fold_pack_enabled()
    monkeypatch.setenv("Y3_FOLD_PACK", "0")
    assert not engine.fold_pack_enabled()
    monkeypatch.setenv("Y3_FOLD_PACK", "1")
    monkeypatch.setattr(engine, "KEEP_FOLDED", True)
    assert not engine.fold_pack_enabled()   # the tests that keep the folded fp32 weights use the per-layer path
    monkeypatch.setattr(engine, "KEEP_FOLDED", False)
    jobs = engine.FoldPackJobs(torch.float16, torch.device("cpu"))
    m = deepcopy(model).eval()
    c0, c2 = m.model[0], m.model[2]
    w0 = jobs.add(c0.conv, c0.bn, True, stem=True)
    w2 = jobs.add(c2.conv, c2.bn, True, cin_pad=16)
    head = m.model[-1].m[0]
    wh = jobs.add(head, None, False)
    assert (w0.cin, w0.cout, w0.k, w0.s, w0.filt.numel()) == (3, 16, 3, 1, 32 * 48)
    assert (w2.cin, w2.cout, w2.filt.numel()) == (16, 32, ops.packed_filter_elems(32, 16, 3)) and w2.bias.shape == (32,)
    assert (wh.cout, wh.filt.numel()) == (24, ops.packed_filter_elems(24, head.in_channels, 1))   # 3 * (3 + 5) = 24 filters
    assert jobs.dirty and jobs.valid() and all(not w.filt.any() and not w.bias.any() for w in (w0, w2, wh))
    c2.conv.weight = torch.nn.Parameter(torch.zeros(8, 16, 3, 3))
    assert not jobs.valid()
