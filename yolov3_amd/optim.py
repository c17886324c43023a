"""Fused SGD(Nesterov) / Adam / AdamW / RMSProp + GradScaler unscale/inf-check + clip_grad_norm_ + ModelEMA on MI355X (csrc/optim.hip).

Mirror of the reference's optimizer step, train.py:414-422:
    scaler.unscale_(optimizer); clip_grad_norm_(model.parameters(), max_norm=10.0); scaler.step(optimizer); ema.update(model)
with the parameter groups of utils/torch_utils.py:207-237 (`smart_optimizer`: biases / BN weights without decay, other
weights with decay, SGD momentum + nesterov).  `param_groups` keeps torch's layout so LR schedulers that write
`group["lr"]` keep working.  No host synchronisation: a step whose gradients contain inf/nan is skipped on the device.
"""
from __future__ import annotations

import math
import struct

import torch
from torch import nn

from . import _lib, ops

CHUNK = 16384


def smart_param_groups(model: nn.Module, lr: float, weight_decay: float):
    """Three groups as reference utils/torch_utils.py:207-237: [weights (decay), norm weights (no decay), biases (no decay)]."""
    bn = tuple(v for k, v in nn.__dict__.items() if "Norm" in k)
    g = [], [], []
    for m in model.modules():
        for name, p in m.named_parameters(recurse=False):
            if name == "bias":
                g[2].append(p)
            elif name == "weight" and isinstance(m, bn):
                g[1].append(p)
            else:
                g[0].append(p)
    return [
        {"params": g[2], "lr": lr, "weight_decay": 0.0},
        {"params": g[0], "lr": lr, "weight_decay": weight_decay},
        {"params": g[1], "lr": lr, "weight_decay": 0.0},
    ]


def freeze_layers(model: nn.Module, freeze) -> list:
    """The reference's --freeze (train.py:217-223): every parameter is set to train, then those whose name contains ``model.{i}.`` for a frozen layer i get
    ``requires_grad = False``.  `freeze` is the command line's list: one element ``[n]`` freezes layers ``range(n)`` (``[10]``: the yolov3 backbone, ``[0]``:
    nothing), a longer list names the layer indices (one layer alone: name it twice, ``[4, 4]``).  Matching is by SUBSTRING of the parameter name, exactly as in
    the reference, so that a run here trains the same parameters as the same command line upstream: the tag may sit anywhere in the name (``module.model.1.`` of a
    wrapped model matches too), and it is the dot behind the index that keeps ``model.1.`` from matching ``model.11.`` or ``model.21.``.  Returns the names of the
    frozen parameters.

    The training engine reads requires_grad when it compiles a step (train_engine.TrainPlan): frozen layers run no backward work, their gradients stay None and
    are not exchanged; they stay in training mode, so their BatchNorm layers keep normalising with batch statistics and updating the running ones, as upstream.
    Build the optimizer after this call (FusedSGD, like the reference's smart_optimizer, takes the parameters that require a gradient)."""
    freeze = list(freeze)
    tags = [f"model.{x}." for x in (freeze if len(freeze) > 1 else range(freeze[0]))]
    frozen = []
    for k, v in model.named_parameters():
        v.requires_grad = True   # train all layers
        if any(x in k for x in tags):
            v.requires_grad = False
            frozen.append(k)
    return frozen


class ModelEMA:
    """Exponential moving average of the model (upstream ultralytics ModelEMA; reference train.py:252,421,437): d = decay * (1 - exp(-updates / tau));
    ema = d * ema + (1 - d) * model, over every floating entry of the state dict.

    ``ema`` is the averaged MODEL, as upstream: a deep copy of the (de-parallelised) model in eval mode whose parameters do not require a gradient -- validate it
    (``run_batches(ema.ema, ..., half=True)``), save it (``compat.save_checkpoint``).  Its parameters and float buffers are the very tensors the kernels lerp into: ``step(ema=ema)`` of a
    fused optimizer is followed by one y3_ema_update_counted launch over all of them, which makes no update when the step was skipped for an inf / nan gradient
    (``after_step``: the update count and the decay live on the device, nothing is read back), and ``update(model)`` is the reference's standalone call: one
    y3_ema_update launch for everything.  ``shadow`` / ``buffers`` map the TRAINING model's parameters / float buffers to their averages.

    The kernels write the averages through raw pointers, which torch's version counters do not see: every update bumps ``ema.weights_epoch`` instead, and the engine
    refills the filter banks of ``ema``'s inference plans when that moved (no plan is rebuilt, nothing is launched here)."""

    def __init__(self, model: nn.Module, decay=0.9999, tau=2000, updates=0):
        from copy import deepcopy

        from .loss import de_parallel

        self.model = model
        self.ema = deepcopy(de_parallel(model)).eval()
        for p in self.ema.parameters():
            p.requires_grad_(False)
            p.grad = None
        self.decay, self.tau = decay, tau
        self._updates, self._state = int(updates), None
        self.rebind(model)

    @property
    def updates(self) -> int:
        """the number of updates made.  After a fused step with ``ema=`` the count lives on the device (a skipped step must not advance it, and only the device knows):
        reading it then synchronises, like GradScaler.get_scale -- for checkpoints and logging."""
        if self._state is not None:
            self._updates = int(self._state[0][:4].view(torch.int32).item())
        return self._updates

    @updates.setter
    def updates(self, value):
        self._updates, self._state = int(value), None   # (the device copy is made again from this value by the next fused step)

    def _device_state(self, device):
        """{int32 updates; float d; double decay; double tau} on `device` (csrc/optim.hip::EmaState), made from the host's values when there is none"""
        key = (device, float(self.decay), float(self.tau))
        if self._state is None or self._state[1] != key:
            n = self.updates
            host = torch.frombuffer(bytearray(struct.pack("<ifdd", n, 0.0, key[1], key[2])), dtype=torch.uint8)
            self._updates, self._state = n, (host.to(device), key)
        return self._state[0]

    def rebind(self, model: nn.Module):
        """(re)build the maps from `model`'s tensors to the averages (after the parameters of either were replaced: ``.to()``, ``.float()``)"""
        from .loss import de_parallel

        m = de_parallel(model)
        self.shadow = dict(zip(m.parameters(), self.ema.parameters()))
        self.buffers = {b: e for b, e in zip(m.buffers(), self.ema.buffers()) if b.dtype.is_floating_point}
        self._tables = {}

    def next_decay(self) -> float:
        """the host's count: ``update(model)`` (no step that could be skipped goes with it)"""
        self.updates += 1
        return self.decay * (1 - math.exp(-self._updates / self.tau))

    def touched(self):
        """the averages were written behind torch's back: make the plan cache of `ema` see a new version (host only)"""
        self.ema.weights_epoch = int(getattr(self.ema, "weights_epoch", 0)) + 1

    def _lerp(self, kind: str, pairs, d: float):
        """ema = d * ema + (1 - d) * src over (src, ema) pairs in one y3_ema_update launch"""
        if not pairs:
            return
        ent = self._table(kind, pairs)
        _lib.check(_lib.lib().y3_ema_update(ent[0].data_ptr(), ent[2], ent[3], float(d), ops.stream_ptr()), "y3_ema_update")

    def _table(self, kind: str, pairs):
        """the device table of (src, ema) records of `kind`; rebuilt only when a tensor moved"""
        ptrs = [t.data_ptr() for pr in pairs for t in pr]
        ent = self._tables.get(kind)
        if ent is None or ent[1] != ptrs:
            rows, n_chunks = [], 0
            for src, dst in pairs:
                ops.require_gpu(dst, "ModelEMA.update")
                if src.dtype != torch.float32 or dst.dtype != torch.float32 or not src.is_contiguous() or not dst.is_contiguous() or src.numel() != dst.numel() or src.device != dst.device:
                    raise TypeError("ModelEMA averages contiguous fp32 tensors (fp32 master weights) that live on the model's device")
                if src.numel() == 0:
                    continue
                rows.append(struct.pack("<QQqii", dst.data_ptr(), src.data_ptr(), src.numel(), n_chunks, 0))
                n_chunks += (src.numel() + CHUNK - 1) // CHUNK
            host = torch.frombuffer(bytearray(b"".join(rows)), dtype=torch.uint8)
            ent = self._tables[kind] = (host.to(pairs[0][1].device), ptrs, len(rows), n_chunks)
        return ent

    @torch.no_grad()
    def update(self, model: nn.Module):
        """The reference's ``ema.update(model)`` after ``scaler.step(optimizer)`` (train.py:421) for loops that do not pass ``ema=`` to the fused step."""
        from .loss import de_parallel

        m = de_parallel(model)
        d = self.next_decay()
        msd, esd = m.state_dict(keep_vars=True), self.ema.state_dict(keep_vars=True)
        self._lerp("all", [(msd[k].detach(), v.detach()) for k, v in esd.items() if v.dtype.is_floating_point], d)
        self.touched()

    def update_buffers(self, d: float):
        self._lerp("buffers", [(b, e) for b, e in self.buffers.items()], d)

    def update_rest(self, d: float, stepped: set):
        """the parameters (`stepped`: ids) the fused step did not touch (frozen ones: no gradient): upstream's ModelEMA.update lerps every float entry of the state dict, so their
        averages still move toward the (unchanged) value -- it matters when the average was loaded from a checkpoint and differs from the weights"""
        self._lerp("rest", [(p.detach(), e) for p, e in self.shadow.items() if id(p) not in stepped], d)

    def after_step(self, found_inf: torch.Tensor):
        """the update that goes with a fused step (``step(ema=ema)``): every parameter -- stepped or frozen -- and every float buffer, in one y3_ema_update_counted
        launch behind the step's kernels.  `found_inf` is the step's DEVICE flag: a step that was skipped for an inf / nan gradient makes NO update -- the averages
        stay bit for bit, buffers included, and the count does not advance, so the next update's decay is that of the updates really made (what a loop gets that
        calls ``ema.update(model)`` only after a step that happened).  Nothing is read back."""
        pairs = [(p.detach(), e) for p, e in self.shadow.items()] + [(b, e) for b, e in self.buffers.items()]
        if not pairs:
            return
        ent = self._table("after_step", pairs)
        state = self._device_state(pairs[0][1].device)
        _lib.check(_lib.lib().y3_ema_update_counted(ent[0].data_ptr(), ent[2], ent[3], state.data_ptr(), found_inf.data_ptr(), ops.stream_ptr()), "y3_ema_update_counted")
        self.touched()

    def update_attr(self, model: nn.Module, include=(), exclude=("process_group", "reducer")):
        """upstream copy_attr (reference train.py:437 ``ema.update_attr(model, include=["yaml", "nc", "hyp", "names", "stride", "class_weights"])``)"""
        for k, v in model.__dict__.items():
            if (len(include) and k not in include) or k.startswith("_") or k in exclude:
                continue
            setattr(self.ema, k, v)


class FusedSGD:
    """torch.optim.SGD(momentum, nesterov) as one fused step.  Every group carries torch's keys ``lr``, ``weight_decay``, ``momentum`` and ``nesterov`` and the step
    reads them there, so a loop that rewrites them between steps -- the reference's warmup, train.py:383-391: ``x["lr"] = ...; if "momentum" in x: x["momentum"] =
    ...`` -- takes effect.  The kernel takes one momentum (and one nesterov flag) per launch: the groups must agree at step time, as they do under that loop."""

    def __init__(self, params, lr=0.01, momentum=0.937, nesterov=True, weight_decay=0.0):
        groups = list(params)
        if groups and not isinstance(groups[0], dict):
            groups = [{"params": groups}]
        self.param_groups = []
        for g in groups:
            g = dict(g)
            g.setdefault("lr", lr)
            g.setdefault("weight_decay", weight_decay)
            g.setdefault("momentum", momentum)
            g.setdefault("nesterov", nesterov)
            g["params"] = [p for p in g["params"] if p.requires_grad]
            self.param_groups.append(g)
        self._defaults = (momentum, nesterov)   # what the properties below answer for an optimizer without groups
        self.state: dict = {}
        self._steps = 0
        self._dev_bufs = None
        self.last_norm = None

    def _agreed(self, key, default):
        """the one value of `key` over the groups (the kernel takes one per launch)"""
        vals = {type(default)(g[key]) for g in self.param_groups}
        if len(vals) > 1:
            raise ValueError(f"FusedSGD keeps one {key} for all groups, the groups have {sorted(vals)}")
        return vals.pop() if vals else default

    @property
    def momentum(self):
        return self._agreed("momentum", float(self._defaults[0]))

    @momentum.setter
    def momentum(self, value):
        for g in self.param_groups:
            g["momentum"] = value

    @property
    def nesterov(self):
        return self._agreed("nesterov", bool(self._defaults[1]))

    @nesterov.setter
    def nesterov(self, value):
        for g in self.param_groups:
            g["nesterov"] = value

    def zero_grad(self, set_to_none=True):
        for g in self.param_groups:
            for p in g["params"]:
                p.grad = None if set_to_none else (p.grad.zero_() if p.grad is not None else None)

    @torch.no_grad()
    def step(self, grad_scale=1.0, max_norm: float = 0.0, ema: ModelEMA | None = None):
        """One fused update.  grad_scale: the loss scale the gradients still carry -- a Python float, or a 1-element DEVICE fp32
        tensor (GradScaler below: dynamic scale, read by the kernels); max_norm: clip_grad_norm_ threshold (0 = off; the
        reference uses 10.0); ema: ModelEMA to update in the same pass.  lr, weight_decay, momentum and nesterov are read from the groups
        now; groups whose momenta (or nesterov flags) differ raise ValueError before anything is launched."""
        momentum, nesterov = self.momentum, self.nesterov
        recs, n_chunks = [], 0
        dev = None
        for g in self.param_groups:
            for p in g["params"]:
                if p.grad is None:
                    continue
                ops.require_gpu(p, "FusedSGD.step")
                if p.dtype != torch.float32 or p.grad.dtype != torch.float32 or not p.is_contiguous():
                    raise TypeError("FusedSGD expects contiguous fp32 master parameters and fp32 gradients")
                dev = p.device
                buf = self.state.get(p)
                if buf is None:
                    buf = self.state[p] = torch.zeros_like(p)
                grad = p.grad.contiguous()
                recs.append((p.data_ptr(), grad.data_ptr(), buf.data_ptr(), 0, p.numel(), float(g["lr"]), float(g["weight_decay"]), n_chunks, grad))
                n_chunks += (p.numel() + CHUNK - 1) // CHUNK
        if not recs:
            return
        L = _lib.lib()
        assert L.y3_sgd_tensor_record_bytes() == 56
        table = b"".join(struct.pack("<QQQQqffii", a, b, c, d, n, lr, wd, fc, 0) for a, b, c, d, n, lr, wd, fc, _ in recs)
        host = torch.frombuffer(bytearray(table), dtype=torch.uint8)
        if self._dev_bufs is None or self._dev_bufs[0].numel() < host.numel() or self._dev_bufs[1].numel() < n_chunks + 2:
            self._dev_bufs = (torch.empty(host.numel(), dtype=torch.uint8, device=dev), torch.empty(n_chunks + 2, dtype=torch.float32, device=dev),
                              torch.zeros(1, dtype=torch.int32, device=dev))
        tab, scratch, found = self._dev_bufs
        tab[: host.numel()].copy_(host, non_blocking=True)
        d = 0.0   # (the kernels' own ema pass is not used: the average follows in ModelEMA.after_step, which knows on the device whether the step was made)
        if isinstance(grad_scale, torch.Tensor):
            if grad_scale.dtype != torch.float32 or grad_scale.numel() != 1 or grad_scale.device != dev:
                raise TypeError("a dynamic loss scale must be a 1-element fp32 tensor on the parameters' device")
            _lib.check(
                L.y3_sgd_step_dynamic(tab.data_ptr(), len(recs), n_chunks, grad_scale.data_ptr(), float(max_norm), float(momentum), int(nesterov),
                                      int(self._steps == 0), float(d), scratch.data_ptr(), found.data_ptr(), ops.stream_ptr()),
                "y3_sgd_step_dynamic",
            )
        else:
            _lib.check(
                L.y3_sgd_step(tab.data_ptr(), len(recs), n_chunks, 1.0 / float(grad_scale), float(max_norm), float(momentum), int(nesterov), int(self._steps == 0),
                              float(d), scratch.data_ptr(), found.data_ptr(), ops.stream_ptr()),
                "y3_sgd_step",
            )
        if ema is not None:
            ema.after_step(found)
        self._steps += 1
        self.last_norm, self.found_inf = scratch[0:1], found  # device tensors; reading them is the caller's (optional) sync

    def state_dict(self):
        """torch.optim.SGD's format: a checkpoint written here loads into torch.optim.SGD(momentum, nesterov) and the other way round"""
        extra = {"dampening": 0, "maximize": False, "foreach": None, "differentiable": False, "fused": None}
        return _pack_state_dict(self.param_groups, extra, lambda p: {"momentum_buffer": self.state[p]} if p in self.state else None)

    def load_state_dict(self, sd):
        saved = _check_groups(self.param_groups, sd)
        mus = {float(g["momentum"]) for g in saved if "momentum" in g}
        if len(mus) > 1:
            raise ValueError(f"FusedSGD keeps one momentum for all groups, the checkpoint has {sorted(mus)}")
        if any(g.get("dampening", 0) != 0 or g.get("maximize", False) for g in saved):
            raise ValueError("FusedSGD does not support dampening / maximize")
        if len({bool(g["nesterov"]) for g in saved if "nesterov" in g}) > 1:
            raise ValueError("FusedSGD keeps one nesterov for all groups, the checkpoint's groups differ")
        _load_groups(self.param_groups, saved, ("lr", "weight_decay", "momentum", "nesterov"))
        self.state = {}
        for p, st in _saved_state(self.param_groups, sd):
            if st.get("momentum_buffer") is not None:
                self.state[p] = st["momentum_buffer"].detach().to(device=p.device, dtype=torch.float32).clone().contiguous()
        # torch takes "first step" per parameter from a missing buffer; here a zero buffer gives the same result (mu * 0 + g), so one loaded buffer ends the first step
        self._steps = 1 if self.state else 0


def _pack_state_dict(groups, extra: dict, state_of):
    """{"state": {index: {...}}, "param_groups": [{..., "params": [indices]}]} -- torch.optim.Optimizer.state_dict()'s layout, parameters numbered in group order"""
    index, out_groups, state = {}, [], {}
    for g in groups:
        d = {k: v for k, v in g.items() if k != "params"}
        for k, v in extra.items():
            d.setdefault(k, v)
        d["params"] = []
        for p in g["params"]:
            i = index.setdefault(id(p), len(index))
            d["params"].append(i)
            st = state_of(p)
            if st is not None:
                state[i] = st
        out_groups.append(d)
    return {"state": state, "param_groups": out_groups}


def _check_groups(groups, sd):
    saved = sd["param_groups"]
    if len(saved) != len(groups):
        raise ValueError("loaded state dict has a different number of parameter groups")
    if any(len(g["params"]) != len(s["params"]) for g, s in zip(groups, saved)):
        raise ValueError("loaded state dict contains a parameter group that doesn't match the size of optimizer's group")
    return saved


def _load_groups(groups, saved, keys):
    for g, s in zip(groups, saved):
        for k in keys:
            if k in s:
                g[k] = tuple(s[k]) if isinstance(s[k], (list, tuple)) else s[k]


def _saved_state(groups, sd):
    """(parameter, its saved state) pairs: the saved indices are matched to this optimizer's parameters by position, as torch does"""
    ids = [i for s in sd["param_groups"] for i in s["params"]]
    params = [p for g in groups for p in g["params"]]
    return [(p, sd["state"][i]) for i, p in zip(ids, params) if i in sd["state"]]


class _FusedMoment:
    """What FusedAdam / FusedAdamW / FusedRMSProp share: torch's param_groups layout (every hyper-parameter is read from its group at every step, so schedulers may
    rewrite them), lazily allocated fp32 state, ONE step counter on the device (it advances only on steps that are not skipped), and the step itself -- the two
    passes of FusedSGD with another update kernel (csrc/optim.hip).  `last_norm` / `found_inf` are device tensors, as FusedSGD's: GradScaler.step drives these too."""

    _what = ""            # class name in messages
    _state_keys = ()      # torch's names of s1, s2

    def _init_groups(self, params, defaults: dict):
        groups = list(params)
        if groups and not isinstance(groups[0], dict):
            groups = [{"params": groups}]
        self.param_groups = []
        for g in groups:
            g = dict(g)
            for k, v in defaults.items():
                g.setdefault(k, v)
            g["params"] = [p for p in g["params"] if p.requires_grad]
            self.param_groups.append(g)
        self.state: dict = {}
        self._step_dev = None       # device int32, the step count t
        self._step_init = 0         # t before the counter exists (load_state_dict on an optimizer that has not stepped)
        self._dev_bufs = None
        self.last_norm = None

    zero_grad = FusedSGD.zero_grad

    def _record(self, g, p):      # -> (s1, s2 or None, h0, h1)
        raise NotImplementedError

    def _launch(self, L, *a):
        raise NotImplementedError

    def _buf(self, p, key):
        st = self.state.setdefault(p, {})
        if key not in st:
            st[key] = torch.zeros_like(p)
        return st[key]

    @torch.no_grad()
    def step(self, grad_scale=1.0, max_norm: float = 0.0, ema: ModelEMA | None = None):
        """One fused update; the arguments are FusedSGD.step's."""
        recs, keep, n_chunks = [], [], 0
        dev = None
        for g in self.param_groups:
            for p in g["params"]:
                if p.grad is None:
                    continue
                ops.require_gpu(p, f"{self._what}.step")
                if p.dtype != torch.float32 or p.grad.dtype != torch.float32 or not p.is_contiguous():
                    raise TypeError(f"{self._what} expects contiguous fp32 master parameters and fp32 gradients")
                dev = p.device
                s1, s2, h0, h1 = self._record(g, p)
                grad = p.grad.contiguous()
                keep.append(grad)
                recs.append(struct.pack("<QQQQQqdddddii", p.data_ptr(), grad.data_ptr(), s1.data_ptr(), s2.data_ptr() if s2 is not None else 0,
                                        0, p.numel(), float(g["lr"]), float(g["weight_decay"]), float(h0), float(h1), float(g["eps"]),
                                        n_chunks, 0))
                n_chunks += (p.numel() + CHUNK - 1) // CHUNK
        if not recs:
            return
        L = _lib.lib()
        assert L.y3_optim_tensor_record_bytes() == 96
        host = torch.frombuffer(bytearray(b"".join(recs)), dtype=torch.uint8)
        if self._dev_bufs is None or self._dev_bufs[0].numel() < host.numel() or self._dev_bufs[1].numel() < n_chunks + 2:
            self._dev_bufs = (torch.empty(host.numel(), dtype=torch.uint8, device=dev), torch.empty(n_chunks + 2, dtype=torch.float32, device=dev),
                              torch.zeros(1, dtype=torch.int32, device=dev))
        if self._step_dev is None:
            self._step_dev = torch.full((1,), self._step_init, dtype=torch.int32, device=dev)
        tab, scratch, found = self._dev_bufs
        tab[: host.numel()].copy_(host, non_blocking=True)
        d = 0.0   # (as in FusedSGD.step: ModelEMA.after_step makes the average's update)
        if isinstance(grad_scale, torch.Tensor):
            if grad_scale.dtype != torch.float32 or grad_scale.numel() != 1 or grad_scale.device != dev:
                raise TypeError("a dynamic loss scale must be a 1-element fp32 tensor on the parameters' device")
            inv, scale_ptr = 1.0, grad_scale.data_ptr()
        else:
            inv, scale_ptr = 1.0 / float(grad_scale), None
        self._launch(L, tab.data_ptr(), len(recs), n_chunks, inv, scale_ptr, float(max_norm), float(d), self._step_dev.data_ptr(), scratch.data_ptr(), found.data_ptr(),
                     ops.stream_ptr())
        if ema is not None:
            ema.after_step(found)
        self.last_norm, self.found_inf = scratch[0:1], found  # device tensors; reading them is the caller's (optional) sync

    def _torch_group_extra(self) -> dict:
        raise NotImplementedError

    def state_dict(self):
        """torch's format (the key names of torch.optim.Adam / AdamW / RMSprop; `step` is a 0-d fp32 CPU tensor, as torch keeps it).  Reads the device step counter:
        synchronises, like GradScaler.get_scale -- for checkpoints only."""
        t = int(self._step_dev.item()) if self._step_dev is not None else self._step_init

        def state_of(p):
            st = self.state.get(p)
            return None if st is None else {"step": torch.tensor(float(t), dtype=torch.float32), **{k: st[k] for k in self._state_keys if k in st}}

        return _pack_state_dict(self.param_groups, self._torch_group_extra(), state_of)

    def _check_flags(self, g):
        raise NotImplementedError

    def load_state_dict(self, sd):
        saved = _check_groups(self.param_groups, sd)
        for g in saved:
            self._check_flags(g)
        pairs = _saved_state(self.param_groups, sd)
        steps = {int(float(st["step"])) for _, st in pairs if "step" in st}
        if len(steps) > 1:
            raise ValueError(f"{self._what} keeps one step counter for all parameters, the checkpoint's `step` values differ: {sorted(steps)}")
        _load_groups(self.param_groups, saved, self._group_keys)
        self.state = {}
        for p, st in pairs:
            self.state[p] = {k: st[k].detach().to(device=p.device, dtype=torch.float32).clone().contiguous() for k in self._state_keys if st.get(k) is not None}
        self._step_init = steps.pop() if steps else 0
        if self._step_dev is not None:
            self._step_dev.fill_(self._step_init)


def _reject(what, **flags):
    for k, v in flags.items():
        if v:
            raise ValueError(f"{what} does not support {k}={v!r}")


class FusedAdam(_FusedMoment):
    """torch.optim.Adam (single-tensor algorithm, fp32 state; amsgrad / maximize unsupported) as one fused step: see _FusedMoment."""

    _what, _decoupled = "FusedAdam", False
    _state_keys = ("exp_avg", "exp_avg_sq")
    _group_keys = ("lr", "betas", "eps", "weight_decay")

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, amsgrad=False, *, maximize=False):
        _reject(self._what, amsgrad=amsgrad, maximize=maximize)
        self._init_groups(params, {"lr": lr, "betas": tuple(betas), "eps": eps, "weight_decay": weight_decay})

    def _record(self, g, p):
        return self._buf(p, "exp_avg"), self._buf(p, "exp_avg_sq"), g["betas"][0], g["betas"][1]

    def _launch(self, L, tab, n, n_chunks, inv, scale_ptr, max_norm, d, step, scratch, found, stream):
        _lib.check(L.y3_adam_step(tab, n, n_chunks, inv, scale_ptr, max_norm, int(self._decoupled), d, step, scratch, found, stream), "y3_adam_step")

    def _torch_group_extra(self):
        return {"amsgrad": False, "maximize": False, "foreach": None, "capturable": False, "differentiable": False, "fused": None, "decoupled_weight_decay": self._decoupled}

    def _check_flags(self, g):
        _reject(self._what, amsgrad=g.get("amsgrad", False), maximize=g.get("maximize", False))


class FusedAdamW(FusedAdam):
    """torch.optim.AdamW: Adam with decoupled weight decay (p *= 1 - lr * wd before the update; torch's default weight_decay 0.01)."""

    _what, _decoupled = "FusedAdamW", True

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, *, maximize=False):
        super().__init__(params, lr, betas, eps, weight_decay, amsgrad, maximize=maximize)


class FusedRMSProp(_FusedMoment):
    """torch.optim.RMSprop (single-tensor algorithm, fp32 state; centered / maximize unsupported) as one fused step: see _FusedMoment.  A group with momentum > 0
    keeps a momentum buffer, one without does not (as torch)."""

    _what = "FusedRMSProp"
    _state_keys = ("square_avg", "momentum_buffer")
    _group_keys = ("lr", "alpha", "eps", "weight_decay", "momentum")

    def __init__(self, params, lr=1e-2, alpha=0.99, eps=1e-8, weight_decay=0.0, momentum=0.0, centered=False, *, maximize=False):
        _reject(self._what, centered=centered, maximize=maximize)
        self._init_groups(params, {"lr": lr, "momentum": momentum, "alpha": alpha, "eps": eps, "weight_decay": weight_decay})

    def _record(self, g, p):
        mu = float(g["momentum"])
        return self._buf(p, "square_avg"), (self._buf(p, "momentum_buffer") if mu > 0 else None), g["alpha"], mu

    def _launch(self, L, tab, n, n_chunks, inv, scale_ptr, max_norm, d, step, scratch, found, stream):
        _lib.check(L.y3_rmsprop_step(tab, n, n_chunks, inv, scale_ptr, max_norm, d, step, scratch, found, stream), "y3_rmsprop_step")

    def _torch_group_extra(self):
        return {"centered": False, "capturable": False, "foreach": None, "maximize": False, "differentiable": False}

    def _check_flags(self, g):
        _reject(self._what, centered=g.get("centered", False), maximize=g.get("maximize", False))


def smart_optimizer(model: nn.Module, name: str = "Adam", lr: float = 0.001, momentum: float = 0.9, decay: float = 1e-5):
    """The optimizer behind the reference's `train.py --optimizer {SGD,Adam,AdamW}` (RMSProp as well), on smart_param_groups' three groups: biases, weights (the only
    group with weight decay), norm weights.  `momentum` is SGD's and RMSProp's momentum and Adam's / AdamW's beta1."""
    groups = smart_param_groups(model, lr, decay)
    if name == "SGD":
        return FusedSGD(groups, lr=lr, momentum=momentum, nesterov=True)
    if name == "Adam":
        return FusedAdam(groups, lr=lr, betas=(momentum, 0.999))
    if name == "AdamW":
        return FusedAdamW(groups, lr=lr, betas=(momentum, 0.999), weight_decay=0.0)
    if name == "RMSProp":
        return FusedRMSProp(groups, lr=lr, momentum=momentum)
    raise NotImplementedError(f"Optimizer {name} not implemented.")


class GradScaler:
    """torch.cuda.amp.GradScaler for the fused optimizer (reference train.py:345 `scaler = torch.cuda.amp.GradScaler(enabled=amp)`,
    :411 `scaler.scale(loss).backward()`, :414-418 `unscale_ / clip_grad_norm_ / step / update`).  The scale, the growth counter and
    the found-inf flag live on the device: `step` hands the scale tensor to the fused kernels (unscale + inf check + clip + SGD +
    EMA in one pass), `update` is one tiny launch -- the loop never synchronises with the host.  Defaults are torch's."""

    def __init__(self, init_scale=2.0**16, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000, enabled=True, device=None):
        self.enabled = enabled
        self.growth_factor, self.backoff_factor, self.growth_interval = float(growth_factor), float(backoff_factor), int(growth_interval)
        self._init_scale, self._device = float(init_scale), device
        self._scale = self._tracker = None
        self._found = None

    def _lazy(self, device):
        if self._scale is None:
            self._scale = torch.full((1,), self._init_scale, dtype=torch.float32, device=device)
            self._tracker = torch.zeros(1, dtype=torch.int32, device=device)

    def scale(self, loss: torch.Tensor) -> torch.Tensor:
        if not self.enabled:
            return loss
        self._lazy(loss.device)
        return loss * self._scale.to(loss.dtype)

    def unscale_(self, optimizer):
        """no separate pass: FusedSGD.step unscales, checks for inf/nan and clips in the same kernels (kept for API parity)"""

    def step(self, optimizer: FusedSGD, max_norm: float = 0.0, ema: ModelEMA | None = None):
        if not self.enabled:
            return optimizer.step(1.0, max_norm, ema)
        p0 = next(p for g in optimizer.param_groups for p in g["params"])
        self._lazy(p0.device)
        optimizer.step(self._scale, max_norm, ema)
        self._found = optimizer.found_inf

    def update(self):
        if not self.enabled or self._found is None:
            return
        _lib.check(_lib.lib().y3_loss_scale_update(self._scale.data_ptr(), self._tracker.data_ptr(), self._found.data_ptr(), self.growth_factor, self.backoff_factor,
                                                   self.growth_interval, ops.stream_ptr()), "y3_loss_scale_update")
        self._found = None

    def get_scale(self) -> float:
        """host read (synchronises): for logging / checkpoints only"""
        return float(self._scale.item()) if self._scale is not None else self._init_scale

    def state_dict(self):
        return {"scale": self.get_scale(), "growth_factor": self.growth_factor, "backoff_factor": self.backoff_factor, "growth_interval": self.growth_interval,
                "_growth_tracker": int(self._tracker.item()) if self._tracker is not None else 0}

    def load_state_dict(self, sd):
        self._init_scale = float(sd["scale"])
        self.growth_factor, self.backoff_factor, self.growth_interval = float(sd["growth_factor"]), float(sd["backoff_factor"]), int(sd["growth_interval"])
        if self._scale is not None:
            self._scale.fill_(self._init_scale)
            self._tracker.fill_(int(sd.get("_growth_tracker", 0)))
