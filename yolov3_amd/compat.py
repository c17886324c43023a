"""Checkpoint ingest for reference ``.pt`` files.

The reference saves PICKLED ``nn.Module`` objects (train.py:470-488: ``{"model": deepcopy(model).half(), "ema": ...}``)
and loads them with ``torch.load`` (models/experimental.py:88-136 ``attempt_load``), which resolves classes by their
qualified names ``models.yolo.DetectionModel``, ``models.yolo.Detect``, ``models.common.Conv`` ...

``attempt_load`` resolves those names through a SCOPED unpickler (``torch.load(pickle_module=...)``): ``find_class`` maps
the reference's qualified names to the yolov3_amd classes for that one load and ``sys.modules`` is never touched, so it
behaves the same in a bare process (the GPU box) and inside a live reference process that has the real ``models.yolo`` /
``models.common`` imported (train.py:50-51, val.py:39, utils/general.py:432).  Whatever the pickle resolved to --
including the reference's own classes when somebody else's ``torch.load`` produced the object -- goes through ``adopt``,
which re-classes the module tree (the attribute names -- ``conv/bn/act``, ``cv1/cv2/add``, ``m/anchors/stride`` -- are
the same) and swaps torch's parameter-free layers for the stand-ins the engine plans with.

``save_checkpoint`` / ``smart_resume`` / ``strip_optimizer`` are the way OUT and back: the reference's checkpoint dict (train.py:470-488), its resume
(utils/torch_utils.py smart_resume) and its final strip (utils/general.py strip_optimizer), over this package's model, ModelEMA and fused optimizers.

``save_reference_checkpoint`` / ``export_reference`` write files that an UNMODIFIED reference process loads (its ``attempt_load``, ``strip_optimizer``,
``smart_resume``): ``to_reference`` gives a copy of the model the attributes the reference's classes expect, and a scoped pickler
(``torch.save(pickle_module=reference_pickle_module())``, the mirror of the scoped unpickler) writes this package's classes under the reference's names.

``install_aliases()`` remains for callers that use a plain ``torch.load`` in a process WITHOUT a reference checkout: it
registers ``models`` / ``models.yolo`` / ``models.common`` / ``models.experimental`` alias modules, and only then: a real
``models`` package that is imported or importable is never shadowed or overwritten.
"""
from __future__ import annotations

import importlib.util
import pickle
import sys
import types

import torch
from torch import nn

from . import common, experimental, yolo

_YOLO_NAMES = ("Detect", "DetectionModel", "Model", "BaseModel", "parse_model")
_COMMON_NAMES = ("Conv", "Bottleneck", "SPP", "Concat", "autopad")
_ALIAS_MODULES = ("models", "models.yolo", "models.common", "models.experimental")


def _class_map() -> dict:
    """qualified reference name -> the class of this package that stands in for it"""
    table = {("models.yolo", n): getattr(yolo, n) for n in _YOLO_NAMES}
    table.update({("models.common", n): getattr(common, n) for n in _COMMON_NAMES})
    table[("models.experimental", "Ensemble")] = experimental.Ensemble
    return table


class _Unpickler(pickle.Unpickler):
    """``find_class`` with the reference's module paths mapped to this package; everything else as usual.  A ``models.*`` class that has
    no MI355X implementation (the unused layer zoo of models/common.py) is refused by name instead of importing whatever
    ``models`` package the process happens to see."""

    def find_class(self, module, name):
        hit = _class_map().get((module, name))
        if hit is not None:
            return hit
        if module in ("models.yolo", "models.common", "models.experimental") or module.startswith("models."):
            raise NotImplementedError(f"checkpoint refers to {module}.{name}, which no yolov3*.yaml uses and which has no MI355X implementation")
        return super().find_class(module, name)


def _pickle_module() -> types.ModuleType:
    """a stand-in for the ``pickle`` module whose Unpickler is the scoped one (what ``torch.load(pickle_module=...)`` expects)"""
    mod = types.ModuleType("yolov3_amd._scoped_pickle")
    mod.__dict__.update({k: v for k, v in pickle.__dict__.items() if not k.startswith("__")})
    mod.Unpickler = _Unpickler

    def load(file, **kw):
        return _Unpickler(file, **kw).load()

    def loads(data, **kw):
        import io

        return _Unpickler(io.BytesIO(data), **kw).load()

    mod.load, mod.loads = load, loads
    return mod


def _real_reference_visible() -> bool:
    """a ``models`` package that is not one of our aliases is imported, or would be found by an import"""
    for name in _ALIAS_MODULES:
        m = sys.modules.get(name)
        if m is not None and not getattr(m, "_yolov3_amd_alias", False):
            return True
    if "models" in sys.modules:          # our alias package
        return False
    try:
        return importlib.util.find_spec("models") is not None
    except (ImportError, ValueError):
        return False


def install_aliases(force: bool = False) -> bool:
    """Make ``models.yolo`` / ``models.common`` importable names for a plain ``torch.load`` in a process without a reference checkout.
    Returns True if the aliases are (now) installed.  Never replaces or shadows a real ``models`` package (``force`` is accepted for
    backward compatibility and re-installs our own aliases only); ``attempt_load`` does not need this."""
    if _real_reference_visible():
        return False
    if not force and all(getattr(sys.modules.get(n), "_yolov3_amd_alias", False) for n in _ALIAS_MODULES):
        return True
    pkg = types.ModuleType("models")
    pkg.__path__ = []
    m_yolo = types.ModuleType("models.yolo")
    m_common = types.ModuleType("models.common")
    m_exp = types.ModuleType("models.experimental")
    for name in _YOLO_NAMES:
        setattr(m_yolo, name, getattr(yolo, name))
    for name in _COMMON_NAMES:
        setattr(m_common, name, getattr(common, name))
    from .autoshape import AutoShape
    from .backend import DetectMultiBackend

    m_common.AutoShape, m_common.DetectMultiBackend = AutoShape, DetectMultiBackend   # utils/general.py:432 imports both
    m_exp.attempt_load, m_exp.Ensemble = attempt_load, experimental.Ensemble
    for m in (pkg, m_yolo, m_common, m_exp):
        m._yolov3_amd_alias = True
    pkg.yolo, pkg.common, pkg.experimental = m_yolo, m_common, m_exp
    sys.modules.update({"models": pkg, "models.yolo": m_yolo, "models.common": m_common, "models.experimental": m_exp})
    return True


def uninstall_aliases():
    """remove the alias modules again (only ours: a real reference package is left alone)"""
    for name in reversed(_ALIAS_MODULES):
        if getattr(sys.modules.get(name), "_yolov3_amd_alias", False):
            del sys.modules[name]


def _reclass(model: nn.Module):
    """objects of the reference's own classes (a model unpickled by somebody else's ``torch.load`` inside a reference process, or built by
    the reference's ``DetectionModel(cfg)``) become objects of this package's classes: same attributes, same parameters, our ``forward``"""
    table = _class_map()
    ours = set(table.values())
    for m in model.modules():
        cls = type(m)
        if cls in ours or not cls.__module__.startswith("models."):
            continue
        hit = table.get((cls.__module__, cls.__name__))
        if hit is None or not isinstance(hit, type):
            raise NotImplementedError(f"{cls.__module__}.{cls.__name__} is not used by any yolov3*.yaml and has no MI355X implementation")
        m.__class__ = hit


def adopt(model: nn.Module) -> nn.Module:
    """Normalise an unpickled reference model: re-class reference objects, swap torch's parameter-free layers for the engine's stand-ins
    and add the attributes newer code expects (mirrors the compatibility loop of models/experimental.py:115-124)."""
    _reclass(model)
    seq = model.model
    for i, m in enumerate(seq):
        new = None
        if isinstance(m, nn.Upsample):
            new = common.Upsample(None, int(m.scale_factor), m.mode)
        elif isinstance(m, nn.MaxPool2d):
            new = common.MaxPool2d(m.kernel_size, m.stride, m.padding)
        elif isinstance(m, nn.ZeroPad2d):
            new = common.ZeroPad2d(list(m.padding))
        if new is not None:
            for a in ("i", "f", "type", "np"):
                if hasattr(m, a):
                    setattr(new, a, getattr(m, a))
            seq[i] = new
    for m in model.modules():
        if isinstance(m, common.Conv):
            c = m.conv
            if c.groups != 1 or c.dilation != (1, 1) or c.kernel_size not in ((1, 1), (3, 3)) or c.stride not in ((1, 1), (2, 2)):
                raise NotImplementedError(f"Conv {c}: the HIP path implements k in (1,3), s in (1,2), g = d = 1 (all yolov3*.yaml shapes)")
            if not isinstance(m.act, (nn.SiLU, nn.Identity)):
                raise NotImplementedError("only SiLU / Identity activations have a fused HIP epilogue")
        if isinstance(m, common.SPP):
            ks = tuple(p.kernel_size for p in getattr(m, "m", [])) or (5, 9, 13)
            if ks != (5, 9, 13):
                raise NotImplementedError(f"SPP kernel sizes {ks}: the HIP pyramid kernel implements (5, 9, 13)")
            m.k = ks
        if isinstance(m, common.Concat) and m.d != 1:
            raise NotImplementedError("Concat along channels only")
        if isinstance(m, nn.SiLU):
            m.inplace = True
    model.__dict__.pop("_plans", None)   # checkpoints written before the plan cache moved out of the module
    return model


_adopt = adopt   # earlier name


def load_checkpoint(weights):
    """``torch.load`` of a reference ``.pt`` with the reference's class paths resolved to this package for this one call"""
    return torch.load(str(weights), map_location="cpu", weights_only=False, pickle_module=_pickle_module())


def attempt_load(weights, device=None, inplace=True, fuse=True):
    """reference models/experimental.py:88-136: per ``.pt`` unpickle, take ``ema`` or ``model``, fp32, fuse, eval.  One weight returns that model; several return an
    ``Ensemble`` with ``names`` / ``nc`` / ``yaml`` of the first member and the ``stride`` of the member whose largest stride is largest.  (``nc``: train.py attaches
    it to the model it saves; a checkpoint without it answers with its Detect head's.)"""
    model = experimental.Ensemble()
    for w in weights if isinstance(weights, (list, tuple)) else [weights]:
        ckpt = load_checkpoint(w)
        ckpt = ckpt.get("ema") or ckpt["model"] if isinstance(ckpt, dict) else ckpt
        ckpt = adopt(ckpt).to(device).float()
        if not hasattr(ckpt, "stride"):
            ckpt.stride = torch.tensor([32.0])
        if hasattr(ckpt, "names") and isinstance(ckpt.names, (list, tuple)):
            ckpt.names = dict(enumerate(ckpt.names))
        model.append(ckpt.fuse().eval() if fuse and hasattr(ckpt, "fuse") else ckpt.eval())
    for m in model.modules():
        if isinstance(m, yolo.Detect):
            m.inplace = inplace
    if len(model) == 1:
        return model[-1]
    for m in model:
        if not hasattr(m, "nc"):
            m.nc = m.model[-1].nc
    for k in "names", "nc", "yaml":
        setattr(model, k, getattr(model[0], k))
    model.stride = model[int(torch.argmax(torch.tensor([float(m.stride.max()) for m in model])))].stride  # max stride
    assert all(model[0].nc == m.nc for m in model), f"Models have different class counts: {[m.nc for m in model]}"
    return model


def _name_map() -> dict:
    """the inverse of ``_class_map``: class (or function) of this package -> the reference's (module, name) for it.  ``Model`` is ``DetectionModel`` under a
    second name on both sides: an object is written under its own ``__name__``."""
    return {obj: key for key, obj in _class_map().items() if getattr(obj, "__name__", None) == key[1]}


class _ReferencePickler(pickle._Pickler):
    """``save_global`` with this package's classes written under the reference's qualified names (``models.yolo.DetectionModel``, ``models.common.Conv`` ...): the
    mirror of ``_Unpickler.find_class``.  The names are WRITTEN, never resolved: nothing is imported, ``sys.modules`` is not read or touched and no class is
    patched, so the stream is the same in a bare process, next to ``install_aliases()`` and inside a live reference process.  A global of this package that has no
    reference name is refused by name: the file would not load in the reference."""

    def save_global(self, obj, name=None):
        hit = _name_map().get(obj) if isinstance(obj, (type, types.FunctionType)) else None
        if hit is None:
            module = getattr(obj, "__module__", None) or ""
            if module == __package__ or module.startswith(__package__ + "."):
                qual = name or getattr(obj, "__qualname__", None) or getattr(obj, "__name__", repr(obj))
                raise pickle.PicklingError(f"{module}.{qual} has no counterpart in the reference (models.yolo / models.common): a file that holds it cannot be "
                                           "loaded there.  Pass plain data (tensors, numbers, str, dict, list) next to the model instead")
            return super().save_global(obj, name)
        module, name = hit
        if self.proto >= 4:
            self.save(module)
            self.save(name)
            self.write(pickle.STACK_GLOBAL)
        else:
            self.write(pickle.GLOBAL + module.encode("ascii") + b"\n" + name.encode("ascii") + b"\n")
        self.memoize(obj)

    # classes come through dispatch[type] (save_type -> self.save_global); functions are dispatched to the function object itself: point that at the override
    dispatch = dict(pickle._Pickler.dispatch)
    dispatch[types.FunctionType] = save_global


def reference_pickle_module() -> types.ModuleType:
    """a stand-in for the ``pickle`` module whose Pickler writes the reference's class names (what ``torch.save(pickle_module=...)`` expects); the mirror of
    ``_pickle_module``.  The pickler is the pure-Python one: tensors leave through torch's persistent ids, so the stream it walks is small."""
    mod = types.ModuleType("yolov3_amd._reference_pickle")
    mod.__dict__.update({k: v for k, v in pickle.__dict__.items() if not k.startswith("__")})
    mod.Pickler = _ReferencePickler

    def dump(obj, file, protocol=None, **kw):
        _ReferencePickler(file, protocol, **kw).dump(obj)

    def dumps(obj, protocol=None, **kw):
        import io

        f = io.BytesIO()
        _ReferencePickler(f, protocol, **kw).dump(obj)
        return f.getvalue()

    mod.dump, mod.dumps = dump, dumps
    return mod


_ENGINE_ONLY = ("_plans", "weights_epoch", "infer_dtype")   # instance attributes the engine reads and the reference does not know


def to_reference(model: nn.Module) -> nn.Module:
    """The inverse of ``adopt``: a deep copy of `model` (wrappers removed) whose objects are still this package's classes and whose attributes are exactly what the
    reference's classes of the same names expect, so that the copy, written with ``reference_pickle_module()``, runs in an unmodified reference process: torch's
    own parameter-free layers in place of the engine's stand-ins, ``SPP.m`` (models/common.py:279), ``Detect.grid`` / ``anchor_grid`` (models/yolo.py:83-84), and
    nothing that exists for the engine alone.  `model` itself -- modules, parameters, compiled plans, filter banks, ``weights_epoch`` -- is not touched."""
    from copy import deepcopy

    from .loss import de_parallel

    model = de_parallel(model)
    if isinstance(model, experimental.Ensemble):
        raise TypeError("an Ensemble is not exported: the reference never pickles one, it builds it in attempt_load from a list of files -- export every member to "
                        "a file of its own and pass the files as `--weights a.pt b.pt`")
    if not isinstance(model, yolo.BaseModel):
        raise TypeError(f"to_reference takes a yolov3_amd detection model, not {type(model).__module__}.{type(model).__name__}")
    if any(isinstance(m, common.Conv) and m.fused for m in model.modules()):
        raise ValueError("a fused model is not exported: the reference's Conv.forward needs `bn` and its loaders fuse for themselves -- export the unfused model "
                         "(the training model, ema.ema, or attempt_load(..., fuse=False))")
    ref = deepcopy(model)
    mapped = set(_name_map())
    for parent in ref.modules():
        for name, m in parent._modules.items():
            new = None
            if type(m) is common.Upsample:
                new = nn.Upsample(None, m.scale_factor, m.mode)
            elif type(m) is common.MaxPool2d:
                new = nn.MaxPool2d(m.kernel_size, m.stride, m.padding)
            elif type(m) is common.ZeroPad2d:
                new = nn.ZeroPad2d(list(m.padding))
            if new is None:
                continue
            for a in ("i", "f", "np"):
                if hasattr(m, a):
                    setattr(new, a, getattr(m, a))
            if hasattr(m, "type"):   # what the reference's parse_model derives from the class: str(nn.Upsample)[8:-2]
                new.type = f"{type(new).__module__}.{type(new).__name__}"
            parent._modules[name] = new
    for m in ref.modules():
        if isinstance(m, common.SPP):
            if not hasattr(m, "m"):
                m.m = nn.ModuleList(nn.MaxPool2d(kernel_size=x, stride=1, padding=x // 2) for x in m.k)
            m.__dict__.pop("k", None)   # (adopt derives it back from `m`)
        if isinstance(m, yolo.Detect):
            for a in ("grid", "anchor_grid"):
                if not isinstance(getattr(m, a, None), list):
                    setattr(m, a, [torch.empty(0) for _ in range(m.nl)])
        for a in _ENGINE_ONLY:
            m.__dict__.pop(a, None)
        for a, v in list(m.__dict__.items()):
            t = type(v)
            if a not in ("_modules", "_parameters", "_buffers") and t.__module__.split(".")[0] == __package__ and t not in mapped:
                del m.__dict__[a]
    return ref


def _save_reference(obj, path):
    """``torch.save`` with the reference's class names, through a temporary file next to `path`: a refused object leaves nothing behind and nothing half-written"""
    import os

    path = str(path)
    tmp = f"{path}.{os.getpid()}.tmp"
    try:
        torch.save(obj, tmp, pickle_module=reference_pickle_module())
        os.replace(tmp, path)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)


def save_reference_checkpoint(path, model, ema, optimizer, epoch, best_fitness=None, **extra):
    """``save_checkpoint`` for a file that the UNMODIFIED reference loads: the same dict (train.py:470-488), ``model`` and ``ema`` passed through ``to_reference`` and
    written under the reference's class names -- for its ``attempt_load`` (detect.py, val.py, export.py, hubconf.custom), ``train.py --weights`` and
    ``smart_resume``.  This package reads the file like any reference checkpoint.  The ``optimizer`` entry is ``optimizer.state_dict()``: torch's format, in the
    group and parameter order of the reference's ``smart_optimizer`` (``smart_param_groups`` is that order); an optimizer built over a model with frozen parameters
    lists the trained ones only, which the reference's ``--resume`` (it lists all) refuses to load.  Returns the dict."""
    ckpt = {
        "epoch": epoch,
        "best_fitness": best_fitness,
        "model": to_reference(model).half(),
        "ema": to_reference(ema.ema).half() if ema is not None else None,
        "updates": ema.updates if ema is not None else None,
        "optimizer": optimizer.state_dict() if optimizer is not None else None,
        **extra,
    }
    _save_reference(ckpt, path)
    return ckpt


def export_reference(src, dst=None):
    """Convert a file written by ``save_checkpoint`` or ``strip_optimizer`` (a full checkpoint or a stripped ``best.pt``) into one the unmodified reference loads;
    everything but ``model`` / ``ema`` goes through as it is.  Written to `dst` (or over `src`); returns the dict."""
    x = load_checkpoint(src)
    if not isinstance(x, dict):
        raise TypeError(f"{src}: expected a checkpoint dict (save_checkpoint / strip_optimizer), got {type(x).__name__}")
    for k in ("model", "ema"):
        if isinstance(x.get(k), nn.Module):
            x[k] = to_reference(x[k])
    _save_reference(x, dst or src)
    return x


def save_checkpoint(path, model, ema, optimizer, epoch, best_fitness=None, **extra):
    """The reference's checkpoint (train.py:470-488): ``{"epoch", "best_fitness", "model": deepcopy(de_parallel(model)).half(), "ema": deepcopy(ema.ema).half(),
    "updates": ema.updates, "optimizer": optimizer.state_dict(), **extra}`` written with ``torch.save``.  The half copies are made with torch on the copies (the
    masters stay fp32); compiled plans live outside the modules and are never pickled.  Returns the dict."""
    from copy import deepcopy

    from .loss import de_parallel

    ckpt = {
        "epoch": epoch,
        "best_fitness": best_fitness,
        "model": deepcopy(de_parallel(model)).half(),
        "ema": deepcopy(ema.ema).half() if ema is not None else None,
        "updates": ema.updates if ema is not None else None,
        "optimizer": optimizer.state_dict() if optimizer is not None else None,
        **extra,
    }
    torch.save(ckpt, str(path))
    return ckpt


def smart_resume(ckpt, optimizer=None, ema=None, weights="", epochs=300, resume=True):
    """reference utils/torch_utils.py smart_resume: restore the optimizer state, the averaged model and its update count from a checkpoint dict (``load_checkpoint``
    reads one); returns (best_fitness, start_epoch, epochs)."""
    best_fitness = 0.0
    start_epoch = ckpt["epoch"] + 1
    if ckpt.get("optimizer") is not None and optimizer is not None:
        optimizer.load_state_dict(ckpt["optimizer"])
        best_fitness = ckpt["best_fitness"] if ckpt.get("best_fitness") is not None else 0.0
    if ema is not None and ckpt.get("ema"):
        ema.ema.load_state_dict(ckpt["ema"].float().state_dict())
        ema.updates = ckpt["updates"]
        ema.touched()   # (load_state_dict copies in place, which torch's version counters see; the bump covers a loader that does not)
    if resume:
        assert start_epoch > 0, f"{weights} training to {epochs} epochs is finished, nothing to resume.\nStart a new training without --resume, i.e. 'python train.py --weights {weights}'"
    if epochs < start_epoch:
        epochs += ckpt["epoch"]   # finetune additional epochs
    return best_fitness, start_epoch, epochs


def strip_optimizer(f="best.pt", s=""):
    """reference utils/general.py strip_optimizer: finalise a checkpoint file -- ``model`` becomes the averaged model, the training state goes, half precision,
    no gradients.  Written to `s` (or over `f`)."""
    x = load_checkpoint(f)
    if x.get("ema"):
        x["model"] = x["ema"]
    for k in ("optimizer", "best_fitness", "ema", "updates"):
        x[k] = None
    x["epoch"] = -1
    x["model"].half()
    for p in x["model"].parameters():
        p.requires_grad = False
    torch.save(x, str(s or f))
    return x
