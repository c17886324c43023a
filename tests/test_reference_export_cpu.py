"""CPU tests of checkpoint EGRESS (compat.to_reference / reference_pickle_module / save_reference_checkpoint / export_reference): the files carry the reference's class
names and nothing of this package, an UNMODIFIED reference process (child processes, skipped where there is no reference tree) loads, runs, strips and resumes
them, this package reads them back bit for bit, the live model is not touched, and what the reference could not read is refused before a byte is written.

Two models: yolov3-tiny nc=3 (the MaxPool2d / ZeroPad2d / Upsample stand-ins) with SGD state, a quarter-width yolov3-spp nc=3 (SPP, Bottleneck) with AdamW state."""
import hashlib
import io
import pickle
import pickletools
import subprocess
import sys
import zipfile
from copy import deepcopy
from pathlib import Path

import pytest
import torch
import yaml
from torch import nn

ROOT = Path(__file__).resolve().parents[1]
NAMES = {0: "cat", 1: "dog", 2: "emu"}
HYP = {"box": 0.05, "cls": 0.5, "anchor_t": 4.0}
CASES = [("tiny", "SGD"), ("spp", "AdamW")]


def _build(kind):
    from yolov3_amd import DetectionModel
    from yolov3_amd.yolo import CFG_DIR

    torch.manual_seed(3)
    if kind == "tiny":
        m = DetectionModel("yolov3-tiny.yaml", nc=3)
    else:
        d = yaml.safe_load((CFG_DIR / "yolov3-spp.yaml").read_text())
        d["width_multiple"] = 0.25
        m = DetectionModel(d, ch=3, nc=3)
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, nn.BatchNorm2d):   # off their initial values: a fold or a buffer that went missing would show
                mod.running_mean.normal_(0, 0.1, generator=g)
                mod.running_var.uniform_(0.5, 1.5, generator=g)
                mod.weight.uniform_(0.8, 1.2, generator=g)
                mod.bias.normal_(0, 0.1, generator=g)
    m.nc, m.names, m.hyp = 3, dict(NAMES), dict(HYP)
    return m


def _objects(kind, opt_name):
    """(model, ModelEMA whose averages differ from the weights, optimizer with a distinct state tensor per parameter); the fused step has no CPU form, so the state
    is assigned directly"""
    from yolov3_amd import ModelEMA, smart_optimizer

    m = _build(kind)
    ema = ModelEMA(m, updates=41)
    with torch.no_grad():
        for p in ema.ema.parameters():
            p.mul_(0.75)
    opt = smart_optimizer(m, opt_name, lr=0.01, momentum=0.9, decay=5e-4)
    g = torch.Generator().manual_seed(11)
    for grp in opt.param_groups:
        for p in grp["params"]:
            if opt_name == "SGD":
                opt.state[p] = torch.randn(p.shape, generator=g)
            else:
                opt.state[p] = {"exp_avg": torch.randn(p.shape, generator=g), "exp_avg_sq": torch.rand(p.shape, generator=g)}
    if opt_name == "SGD":
        opt._steps = 1
    else:
        opt._step_init = 7
    return m, ema, opt


def _state_by_name(m, opt, opt_name):
    out = {}
    for n, p in m.named_parameters():
        st = opt.state[p]
        out[n] = {"momentum_buffer": st.clone()} if opt_name == "SGD" else {"step": torch.tensor(7.0), **{k: v.clone() for k, v in st.items()}}
    return out


@pytest.fixture(scope="module", params=CASES, ids=[f"{k}-{o}" for k, o in CASES])
def saved(request, tmp_path_factory):
    """one exported checkpoint per case, and next to it (plain tensors and containers) what the reference child processes compare against"""
    from yolov3_amd import save_reference_checkpoint

    kind, opt_name = request.param
    d = tmp_path_factory.mktemp(f"export_{kind}")
    m, ema, opt = _objects(kind, opt_name)
    ck = save_reference_checkpoint(d / "last.pt", m, ema, opt, epoch=4, best_fitness=0.25, date="today")
    want = {
        "opt": _state_by_name(m, opt, opt_name),
        "ema": {k: v.half().float() if v.is_floating_point() else v.clone() for k, v in ema.ema.state_dict().items()},
        "updates": 41, "yaml": deepcopy(m.yaml), "hyp": dict(HYP), "names": dict(NAMES), "stride": m.stride.tolist(),
    }
    torch.save(want, d / "want.pt")
    return {"kind": kind, "opt": opt_name, "dir": d, "f": d / "last.pt", "want": d / "want.pt", "m": m, "ema": ema, "optimizer": opt, "ck": ck}


def _data_pkl(f) -> bytes:
    with zipfile.ZipFile(f) as z:
        return z.read(next(n for n in z.namelist() if n.endswith("/data.pkl")))


def _stream_names(data: bytes):
    """every global of a pickle stream as (module, name); no string argument may begin with this package's name.  (GLOBAL carries both strings; STACK_GLOBAL takes
    them from the stack, where a repeated string is a memo read: the last two string pushes are tracked through the memo.)"""
    found, pushed, memo, last = [], [], {}, None
    for op, arg, _ in pickletools.genops(data):
        if isinstance(arg, str):
            assert not arg.startswith("yolov3_amd"), f"{op.name} {arg!r}"
        if op.name in ("GLOBAL", "INST"):
            found.append(tuple(arg.split(" ", 1)))
        elif op.name == "STACK_GLOBAL":
            found.append(tuple(pushed[-2:]))
        if op.name in ("BINUNICODE", "SHORT_BINUNICODE", "BINUNICODE8", "UNICODE"):
            pushed.append(arg)
            last = arg
        elif op.name in ("BINGET", "LONG_BINGET", "GET"):
            last = memo.get(int(arg))
            if isinstance(last, str):
                pushed.append(last)
        elif op.name in ("BINPUT", "LONG_BINPUT", "PUT"):
            memo[int(arg)] = last
        elif op.name == "MEMOIZE":
            memo[len(memo)] = last
        else:
            last = None
    return found


def _check_stream(data: bytes):
    from yolov3_amd import compat

    names = _stream_names(data)
    assert all(not mod.startswith("yolov3_amd") for mod, _ in names)
    ours = [n for n in names if n[0] == "models" or n[0].startswith("models.")]
    assert ours and all(n in compat._class_map() for n in ours), ours
    return set(ours)


def _run_py(code, cwd):
    r = subprocess.run([sys.executable, "-c", code], cwd=cwd, text=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout
    return r.stdout


def _need_reference():
    from oracle import ref_shim

    if not ref_shim.available():
        pytest.skip("reference tree not present on this box")


# a child process with nothing but the UNMODIFIED reference imported.  ref_shim binds ultralytics' torch_load to plain torch.load; upstream's passes weights_only=False
LIVE = f"""
import sys, functools, torch
sys.path.insert(0, {str(ROOT)!r})
from oracle import ref_shim
ref_shim.install()
import models.experimental, models.yolo, utils.general, utils.torch_utils
load = functools.partial(torch.load, weights_only=False)
models.experimental.torch_load = utils.general.torch_load = load
assert not any(k == 'yolov3_amd' or k.startswith('yolov3_amd.') for k in sys.modules)
"""


# ------------------------------------------------------------------------------------------------ the stream
def test_public_names():
    import inspect

    import yolov3_amd
    from yolov3_amd import compat

    for n in ("to_reference", "reference_pickle_module", "save_reference_checkpoint", "export_reference"):
        assert getattr(yolov3_amd, n) is getattr(compat, n)
    assert list(inspect.signature(compat.save_reference_checkpoint).parameters) == list(inspect.signature(compat.save_checkpoint).parameters)
    assert list(inspect.signature(compat.export_reference).parameters) == ["src", "dst"]


def test_stream_holds_reference_names_only(saved):
    from yolov3_amd import compat

    whole = _check_stream(_data_pkl(saved["f"]))
    want = {("models.yolo", "DetectionModel"), ("models.yolo", "Detect"), ("models.common", "Conv"), ("models.common", "Concat")}
    want |= {("models.common", "SPP"), ("models.common", "Bottleneck")} if saved["kind"] == "spp" else set()
    assert whole == want
    for k in ("model", "ema"):   # each object on its own
        buf = io.BytesIO()
        torch.save(saved["ck"][k], buf, pickle_module=compat.reference_pickle_module())
        assert _check_stream(_data_pkl(buf)) == want
    assert set(saved["ck"]) == {"epoch", "best_fitness", "model", "ema", "updates", "optimizer", "date"}


def test_pickler_writes_both_global_forms_and_functions():
    from yolov3_amd import Conv, DetectionModel, Model, compat, parse_model

    pm = compat.reference_pickle_module()
    for proto in (2, 3, 4, 5):
        data = pm.dumps([Conv, DetectionModel, Model, parse_model, Conv], protocol=proto)
        assert _stream_names(data) == [("models.common", "Conv"), ("models.yolo", "DetectionModel"), ("models.yolo", "parse_model")], proto   # repeats are memo reads
    assert pickle.loads(pm.dumps({"a": (1, 2.5, "x"), "t": torch.float16})) == {"a": (1, 2.5, "x"), "t": torch.float16}   # everything else as usual


# ------------------------------------------------------------------------------------------------ the live reference
def test_unmodified_reference_loads_runs_and_strips(saved, tmp_path):
    from yolov3_amd import DetectionModel, attempt_load

    _need_reference()
    s = tmp_path / "best.pt"
    code = LIVE + f"""
import yaml
kind, f, s = {saved['kind']!r}, {str(saved['f'])!r}, {str(s)!r}
want = torch.load({str(saved['want'])!r})
m = models.experimental.attempt_load(f, device='cpu', fuse=False)
assert type(m) is models.yolo.DetectionModel and not m.training and next(m.parameters()).dtype == torch.float32
assert type(m.model[-1]) is models.yolo.Detect and isinstance(m.model[-1].anchor_grid, list)
cfg = ref_shim.REFERENCE_ROOT / 'models' / ('yolov3-tiny.yaml' if kind == 'tiny' else 'yolov3-spp.yaml')
if kind == 'spp':
    cfg = yaml.safe_load(cfg.read_text())
    cfg['width_multiple'] = 0.25
else:
    cfg = str(cfg)
ref = models.yolo.DetectionModel(cfg, ch=3, nc=3)
ref.load_state_dict(m.state_dict(), strict=True)
ref.eval()
sd = m.state_dict()
assert set(sd) == set(want['ema']) and all(torch.equal(v, want['ema'][k]) for k, v in sd.items())   # attempt_load prefers the averaged model
x = torch.rand(2, 3, 64, 96, generator=torch.Generator().manual_seed(1))
with torch.no_grad():
    a, b = m(x), ref(x)
    assert a[0].shape[0] == 2 and a[0].shape[2] == 8 and torch.equal(a[0], b[0]) and len(a[1]) == len(b[1]) and all(torch.equal(p, q) for p, q in zip(a[1], b[1]))
    fused = models.experimental.attempt_load(f, device='cpu', fuse=True)
    assert not any(hasattr(c, 'bn') for c in fused.modules() if type(c) is models.common.Conv)
    y = fused(x)[0]
    assert y.shape == a[0].shape and bool(torch.isfinite(y).all())
for md in (m, fused):
    assert md.names == want['names'] and md.hyp == want['hyp'] and md.yaml == want['yaml'] and md.stride.tolist() == want['stride'] and md.nc == 3
utils.general.strip_optimizer(f, s)
x2 = load(s, map_location='cpu')
assert type(x2['model']) is models.yolo.DetectionModel and x2['ema'] is None and x2['optimizer'] is None and x2['epoch'] == -1
assert all(p.dtype == torch.float16 and not p.requires_grad for p in x2['model'].parameters())
ms = models.experimental.attempt_load(s, device='cpu', fuse=False)
assert type(ms) is models.yolo.DetectionModel and all(torch.equal(v, sd[k]) for k, v in ms.state_dict().items())
print('ok')
"""
    _run_py(code, tmp_path)
    # what the reference's strip_optimizer wrote loads here as any reference file does
    _check_stream(_data_pkl(s))
    got = attempt_load(s, device="cpu", fuse=False)
    want = torch.load(saved["want"])["ema"]
    assert type(got) is DetectionModel and set(got.state_dict()) == set(want) and all(torch.equal(v, want[k]) for k, v in got.state_dict().items())


def test_unmodified_reference_resumes(saved, tmp_path):
    """the reference's smart_optimizer on the loaded fp32 model, its smart_resume: every state tensor lands on the parameter of the same NAME, the averaged model and its
    update count come back.  (ModelEMA is ultralytics', which the reference tree does not hold: the holder below has the two attributes smart_resume uses.)"""
    _need_reference()
    code = LIVE + f"""
from copy import deepcopy
f, name = {str(saved['f'])!r}, {saved['opt']!r}
want = torch.load({str(saved['want'])!r})
ck = load(f, map_location='cpu')
model = ck['model'].float()
opt = utils.torch_utils.smart_optimizer(model, name, lr=0.5, momentum=0.3, decay=0.0)
assert type(opt) is (torch.optim.SGD if name == 'SGD' else torch.optim.AdamW)
class EMA:
    def __init__(self, model):
        self.ema, self.updates = deepcopy(model).eval(), 0
ema = EMA(model)
assert utils.torch_utils.smart_resume(ck, opt, ema, weights=f, epochs=300, resume=True) == (0.25, 5, 300)
params = dict(model.named_parameters())
assert set(params) == set(want['opt']) and len(opt.state) == len(params)
for n, p in params.items():
    st = opt.state[p]
    assert set(st) == set(want['opt'][n]), (n, set(st))
    for k, v in want['opt'][n].items():
        assert st[k].shape == v.shape and torch.equal(st[k].float(), v), (n, k)
assert [g['weight_decay'] for g in opt.param_groups] == [0.0, 5e-4, 0.0] and all(g['lr'] == 0.01 for g in opt.param_groups)
assert all(g['momentum'] == 0.9 and g['nesterov'] for g in opt.param_groups) if name == 'SGD' else all(tuple(g['betas']) == (0.9, 0.999) for g in opt.param_groups)
assert ema.updates == want['updates'] == 41
sd = ema.ema.state_dict()
assert set(sd) == set(want['ema']) and all(torch.equal(v, want['ema'][k]) for k, v in sd.items())
print('ok')
"""
    _run_py(code, tmp_path)


# ------------------------------------------------------------------------------------------------ one stream in every kind of process
SAVE_IN_CHILD = """
import hashlib, zipfile
from yolov3_amd import ModelEMA, compat, save_reference_checkpoint, smart_optimizer
before = {k: v for k, v in sys.modules.items() if k == 'models' or k.startswith('models.')}
ck = compat.load_checkpoint(SRC)
m = ck['model'].float()
ema = ModelEMA(ck['ema'].float(), updates=ck['updates'])
opt = smart_optimizer(m, 'SGD')
opt.load_state_dict(ck['optimizer'])
save_reference_checkpoint(DST, m, ema, opt, epoch=ck['epoch'], best_fitness=ck['best_fitness'], date=ck['date'])
after = {k: v for k, v in sys.modules.items() if k == 'models' or k.startswith('models.')}
assert set(before) == set(after) and all(before[k] is after[k] for k in before), (sorted(before), sorted(after))
with zipfile.ZipFile(DST) as z:
    print(len(before), hashlib.sha256(z.read(next(n for n in z.namelist() if n.endswith('/data.pkl')))).hexdigest(), 'ok')
"""


def test_same_stream_bare_with_aliases_and_in_a_live_reference_process(tmp_path):
    from yolov3_amd import save_checkpoint

    m, ema, opt = _objects("tiny", "SGD")
    src = tmp_path / "src.pt"
    save_checkpoint(src, m, ema, opt, epoch=4, best_fitness=0.25, date="today")
    head = f"import sys, torch\nsys.path.insert(0, {str(ROOT)!r})\nSRC = {str(src)!r}\n"
    settings = {
        "bare": "",
        "aliases": "from yolov3_amd import compat as c0\nassert c0.install_aliases() and 'models.yolo' in sys.modules\n",
    }
    from oracle import ref_shim

    if ref_shim.available():
        settings["live"] = "from oracle import ref_shim\nref_shim.load()\nimport models.yolo, models.common, models.experimental\nassert not hasattr(sys.modules['models'], '_yolov3_amd_alias')\n"
    digests = {}
    for name, setup in settings.items():
        out = _run_py(head + f"DST = {str(tmp_path / (name + '.pt'))!r}\n" + setup + SAVE_IN_CHILD, tmp_path).split()
        digests[name] = out[-2]
        assert (int(out[-3]) == 0) == (name == "bare")
        assert _data_pkl(tmp_path / (name + ".pt")) and hashlib.sha256(_data_pkl(tmp_path / (name + ".pt"))).hexdigest() == out[-2]
    assert len(set(digests.values())) == 1, digests
    _check_stream(_data_pkl(tmp_path / "bare.pt"))
    if "live" not in settings:
        pytest.skip("reference tree not present on this box: the bare and the alias settings agree, the live one did not run")


# ------------------------------------------------------------------------------------------------ this package reads its own exports
def _equal_state(a, b):
    a, b = a.state_dict(), b.state_dict()
    return list(a) == list(b) and all(torch.equal(v, b[k]) and v.dtype == b[k].dtype for k, v in a.items())


def test_own_loader_reads_the_export_like_a_reference_file(saved, tmp_path):
    from yolov3_amd import DetectionModel, ModelEMA, attempt_load, common, compat, smart_optimizer, smart_resume, strip_optimizer

    ck = compat.load_checkpoint(saved["f"])
    assert set(ck) == set(saved["ck"]) and (ck["epoch"], ck["best_fitness"], ck["updates"], ck["date"]) == (4, 0.25, 41, "today")
    for k, live in (("model", saved["m"]), ("ema", saved["ema"].ema)):
        assert type(ck[k]) is DetectionModel and _equal_state(ck[k], saved["ck"][k]) and _equal_state(ck[k], deepcopy(live).half())
    got = attempt_load(saved["f"], device="cpu", fuse=False)
    assert type(got) is DetectionModel and _equal_state(got, deepcopy(saved["ema"].ema).half().float())
    kinds = {type(x) for x in got.model}
    assert not kinds & {nn.Upsample, nn.MaxPool2d, nn.ZeroPad2d} and common.Upsample in kinds   # adopted: the engine's stand-ins are back
    assert all(x.k == (5, 9, 13) for x in got.modules() if isinstance(x, common.SPP))
    assert type(attempt_load(saved["f"], device="cpu")) is DetectionModel   # fused
    # resume into fresh objects
    m2 = _build(saved["kind"])
    ema2, opt2 = ModelEMA(m2), smart_optimizer(m2, saved["opt"], lr=0.5, momentum=0.3, decay=0.0)
    assert smart_resume(ck, opt2, ema2, weights="last.pt", epochs=300, resume=True) == (0.25, 5, 300)
    assert ema2.updates == 41 and _equal_state(ema2.ema, deepcopy(saved["ema"].ema).half().float())
    want = _state_by_name(saved["m"], saved["optimizer"], saved["opt"])
    for n, p in m2.named_parameters():
        st = opt2.state[p]
        assert torch.equal(st, want[n]["momentum_buffer"]) if saved["opt"] == "SGD" else all(torch.equal(st[k], want[n][k]) for k in ("exp_avg", "exp_avg_sq")), n
    assert saved["opt"] == "SGD" or opt2._step_init == 7
    # strip
    s = tmp_path / "best.pt"
    x = strip_optimizer(saved["f"], s)
    assert x["ema"] is None and x["optimizer"] is None and x["epoch"] == -1 and _equal_state(compat.load_checkpoint(s)["model"], saved["ck"]["ema"])


def test_round_trip_through_export_reference(saved, tmp_path):
    from yolov3_amd import DetectionModel, attempt_load, compat, export_reference, save_checkpoint, strip_optimizer

    f0, f1, f2 = tmp_path / "ours.pt", tmp_path / "export.pt", tmp_path / "again.pt"
    save_checkpoint(f0, saved["m"], saved["ema"], saved["optimizer"], epoch=4, best_fitness=0.25, date="today")
    with pytest.raises(AssertionError):
        _check_stream(_data_pkl(f0))   # what save_checkpoint writes names this package
    x = export_reference(f0, f1)
    assert f0.exists() and set(x) == set(saved["ck"])
    export_reference(f1, f2)   # load_checkpoint -> to_reference -> save, on a file that is already an export
    assert _check_stream(_data_pkl(f1)) == _check_stream(_data_pkl(f2)) == _check_stream(_data_pkl(saved["f"]))
    c0, c1, c2 = (compat.load_checkpoint(f) for f in (f0, f1, f2))
    for k in ("model", "ema"):
        assert _equal_state(c0[k], c1[k]) and _equal_state(c0[k], c2[k])
    for a, b in zip(c0["optimizer"]["state"].values(), c2["optimizer"]["state"].values()):
        assert all(torch.equal(torch.as_tensor(a[k]), torch.as_tensor(b[k])) for k in a)
    assert c0["optimizer"]["param_groups"] == c2["optimizer"]["param_groups"]
    assert type(attempt_load(f2, device="cpu")) is DetectionModel
    # a stripped best.pt, converted in place
    s = tmp_path / "best.pt"
    strip_optimizer(f0, s)
    export_reference(s)
    _check_stream(_data_pkl(s))
    y = compat.load_checkpoint(s)
    assert y["epoch"] == -1 and y["ema"] is None and _equal_state(y["model"], c0["ema"]) and all(not p.requires_grad for p in y["model"].parameters())
    assert not [p.name for p in tmp_path.iterdir() if p.name.endswith(".tmp")]


# ------------------------------------------------------------------------------------------------ to_reference
def test_to_reference_builds_what_the_reference_classes_expect_and_leaves_the_model_alone(saved):
    from yolov3_amd import Detect, DetectionModel, ModelEMA, common, to_reference

    m = deepcopy(saved["m"])
    m.infer_dtype = torch.float16            # engine-only instance attributes
    m.weights_epoch = 3
    m.helper = ModelEMA.__new__(ModelEMA)    # an object of a class the reference has no name for
    mods, params, keys = [id(x) for x in m.modules()], [id(p) for p in m.parameters()], {id(x): set(vars(x)) for x in m.modules()}
    before = deepcopy(m.state_dict())
    ref = to_reference(m)
    # the live model: same objects, same attributes, our stand-ins, no grid
    assert [id(x) for x in m.modules()] == mods and [id(p) for p in m.parameters()] == params and all(set(vars(x)) == keys[id(x)] for x in m.modules())
    assert m.infer_dtype == torch.float16 and m.weights_epoch == 3 and isinstance(m.helper, ModelEMA)
    assert not hasattr(m.model[-1], "grid") and not hasattr(m.model[-1], "anchor_grid")
    assert not any(isinstance(x, (nn.Upsample, nn.MaxPool2d, nn.ZeroPad2d)) for x in m.modules())
    assert all(torch.equal(v, before[k]) for k, v in m.state_dict().items())
    # the copy
    assert type(ref) is DetectionModel and ref is not m and _equal_state(ref, m)
    assert not {id(p) for p in ref.parameters()} & set(params)
    assert not any(isinstance(x, (common.Upsample, common.MaxPool2d, common.ZeroPad2d)) for x in ref.modules())
    assert all(k not in vars(ref) for k in ("infer_dtype", "weights_epoch", "helper", "_plans"))
    assert ref.names == NAMES and ref.hyp == HYP and ref.yaml == m.yaml and torch.equal(ref.stride, m.stride) and ref.save == m.save
    for a, b in zip(m.model, ref.model):
        assert (a.i, a.f, a.np) == (b.i, b.f, b.np)
        if type(a) is common.Upsample:
            assert type(b) is nn.Upsample and (b.size, b.scale_factor, b.mode, b.type) == (None, 2.0, "nearest", "torch.nn.modules.upsampling.Upsample")
        elif type(a) is common.MaxPool2d:
            assert type(b) is nn.MaxPool2d and (b.kernel_size, b.stride, b.padding, b.type) == (a.kernel_size, a.stride, a.padding, "torch.nn.modules.pooling.MaxPool2d")
        elif type(a) is common.ZeroPad2d:
            assert type(b) is nn.ZeroPad2d and list(b.padding) == [0, 1, 0, 1] and b.type == "torch.nn.modules.padding.ZeroPad2d"
        else:
            assert type(a) is type(b) and a.type == b.type
    kinds = {type(x) for x in ref.model}
    assert kinds >= ({nn.Upsample, nn.MaxPool2d, nn.ZeroPad2d} if saved["kind"] == "tiny" else {nn.Upsample, common.SPP, common.Bottleneck})
    for x in ref.modules():
        if isinstance(x, common.SPP):
            assert "k" not in vars(x) and [(p.kernel_size, p.stride, p.padding) for p in x.m] == [(5, 1, 2), (9, 1, 4), (13, 1, 6)] and list(x._modules) == ["cv1", "cv2", "m"]
    d = ref.model[-1]
    assert type(d) is Detect and all(isinstance(g, list) and len(g) == d.nl and all(t.numel() == 0 for t in g) for g in (d.grid, d.anchor_grid))
    # wrappers are removed; a reference-shaped copy converts again to the same thing
    assert type(to_reference(nn.DataParallel(m))) is DetectionModel
    again = to_reference(ref)
    assert _equal_state(again, ref) and [type(x) for x in again.modules()] == [type(x) for x in ref.modules()]


def test_refusals_leave_no_file(saved, tmp_path):
    from yolov3_amd import Ensemble, ModelEMA, general, save_reference_checkpoint, to_reference

    m, ema, opt = saved["m"], saved["ema"], saved["optimizer"]
    f = tmp_path / "last.pt"

    def nothing_written():
        return not f.exists() and list(tmp_path.iterdir()) == []

    ens = Ensemble([deepcopy(m).eval(), deepcopy(m).eval()])
    with pytest.raises(TypeError, match="export every member"):
        to_reference(ens)
    with pytest.raises(TypeError, match="export every member"):
        save_reference_checkpoint(f, ens, ema, opt, epoch=0)
    assert nothing_written()
    fused = deepcopy(m).eval().fuse()
    with pytest.raises(ValueError, match="export the unfused model"):
        to_reference(fused)
    with pytest.raises(ValueError, match="export the unfused model"):
        save_reference_checkpoint(f, fused, None, None, epoch=0)
    with pytest.raises(TypeError, match="detection model"):
        to_reference(nn.Conv2d(3, 3, 1))
    assert nothing_written()
    # an object graph that holds a class (or a function) of this package without a reference name
    with pytest.raises(pickle.PicklingError, match=r"yolov3_amd\.optim\.ModelEMA has no counterpart"):
        save_reference_checkpoint(f, m, ema, opt, epoch=0, trainer={"ema": ModelEMA.__new__(ModelEMA)})
    assert nothing_written()
    with pytest.raises(pickle.PicklingError, match=r"yolov3_amd\.general\.xywh2xyxy has no counterpart"):
        save_reference_checkpoint(f, m, ema, opt, epoch=0, box_fn=general.xywh2xyxy)
    deep = deepcopy(m)
    deep.hyp = {"nested": [ModelEMA]}   # below the attributes to_reference looks at: the pickler's to refuse
    with pytest.raises(pickle.PicklingError, match=r"yolov3_amd\.optim\.ModelEMA has no counterpart"):
        save_reference_checkpoint(f, deep, None, None, epoch=0)
    assert nothing_written()
    # a refused save over an existing file leaves that file as it was
    f.write_bytes(b"earlier")
    with pytest.raises(pickle.PicklingError):
        save_reference_checkpoint(f, m, ema, opt, epoch=0, box_fn=general.xywh2xyxy)
    assert f.read_bytes() == b"earlier" and [p.name for p in tmp_path.iterdir()] == ["last.pt"]
    save_reference_checkpoint(f, m, ema, opt, epoch=0)
    _check_stream(_data_pkl(f))
