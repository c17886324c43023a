"""Thin host wrappers over the C ABI (include/yolov3_hip.h): torch supplies device memory and the stream,
nothing else.  Activations are NHWC views (`View`) over flat torch buffers."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import NamedTuple

import math

import torch

from . import _lib
from ._lib import Y3AugmentItem, Y3AugmentMosaic, Y3AugmentTile, Y3ConvDesc, Y3DatasetImage, Y3NmsParams, Y3Tensor, check   # (the record structs: for dataset.py / augment.py)

DTYPE_CODE = {torch.float16: _lib.Y3_F16, torch.bfloat16: _lib.Y3_BF16, torch.float32: _lib.Y3_F32, torch.uint8: _lib.Y3_U8}


def dtype_code(dt: torch.dtype) -> int:
    try:
        return DTYPE_CODE[dt]
    except KeyError:
        raise TypeError(f"dtype {dt} is not supported by the MI355X path (float16 / bfloat16 / float32)") from None


def require_gpu(t: torch.Tensor, what: str):
    if not t.is_cuda:
        raise RuntimeError(
            f"{what}: tensor is on {t.device}; the yolov3_amd hot path runs only on an MI355X (HIP) device. "
            "There is no CPU / PyTorch fallback."
        )


def stream_ptr() -> int:
    return torch.cuda.current_stream().cuda_stream


def tune_set(key: str, value: int):
    """run-time knob of the library (y3_tune_set: A/B hooks, test coverage of size-gated forms); process-wide"""
    check(_lib.lib().y3_tune_set(key.encode(), int(value)), "y3_tune_set")


def tune_get(key: str) -> int:
    v = _lib.lib().y3_tune_get(key.encode())
    if v == -(2**63):
        raise _lib.Y3Error(_lib.lib().y3_last_error().decode(errors="replace"))
    return int(v)


def tune_reset():
    _lib.lib().y3_tune_reset()


@dataclass
class View:
    """NHWC view: channels [coff, coff+c) of a (n, h, w, pitch) buffer."""

    buf: torch.Tensor  # flat storage, at least n*h*w*pitch elements
    n: int
    h: int
    w: int
    c: int
    pitch: int
    coff: int = 0

    def y3(self) -> Y3Tensor:
        ptr = self.buf.data_ptr() + self.coff * self.buf.element_size()
        return Y3Tensor(ptr, self.n, self.h, self.w, self.c, self.pitch)

    def slice(self, coff: int, c: int) -> "View":
        assert coff + c <= self.c
        return View(self.buf, self.n, self.h, self.w, c, self.pitch, self.coff + coff)

    def as_nhwc(self) -> torch.Tensor:
        """torch view (n,h,w,c) for tests/debug."""
        full = self.buf[: self.n * self.h * self.w * self.pitch].view(self.n, self.h, self.w, self.pitch)
        return full[..., self.coff : self.coff + self.c]

    @staticmethod
    def alloc(n, h, w, c, dtype, device, pitch=None) -> "View":
        pitch = pitch or c
        return View(torch.empty(n * h * w * pitch, dtype=dtype, device=device), n, h, w, c, pitch, 0)


def _ptr(t: torch.Tensor | None):
    return t.data_ptr() if t is not None else None


def _ref(v: View | None):
    return C.byref(v.y3()) if v is not None else None


def packed_filter_elems(cout: int, cin: int, k: int) -> int:
    return int(_lib.lib().y3_packed_filter_elems(cout, cin, k))


def pack_filter(w_oihw: torch.Tensor, cout: int, cin: int, dtype: torch.dtype) -> torch.Tensor:
    """OIHW fp32 weights (device) -> packed filter bank for y3_conv2d_fwd, zero padded to (cout, cin)."""
    require_gpu(w_oihw, "pack_filter")
    w = w_oihw.detach().to(torch.float32).contiguous()
    co, ci, k, _ = w.shape
    out = torch.empty(packed_filter_elems(cout, cin, k), dtype=dtype, device=w.device)
    check(_lib.lib().y3_pack_filter(w.data_ptr(), co, ci, k, cout, cin, dtype_code(dtype), out.data_ptr(), stream_ptr()), "y3_pack_filter")
    return out


def conv_workspace(device) -> torch.Tensor:
    """Scratch of the K-split form of the persistent 3x3 kernel (y3_conv2d_fwd_ws: fp32 slabs for small launches): allocated once here, owned by whoever runs convs on ONE
    stream at a time (a compiled plan keeps its own)."""
    return torch.zeros(int(_lib.lib().y3_conv_workspace_bytes()), dtype=torch.uint8, device=device)


def conv2d(x: View, filt: torch.Tensor, bias: torch.Tensor, y: View, k: int, stride: int, act: bool, residual: View | None = None, upsample2x: bool = False,
           algo: int = _lib.Y3_ALGO_AUTO, in_dilation: int = 0, workspace: torch.Tensor | None = None):
    d = Y3ConvDesc(dtype_code(x.buf.dtype), k, stride, _lib.Y3_ACT_SILU if act else _lib.Y3_ACT_NONE, int(upsample2x), algo, x.c, y.c, in_dilation, filt.numel())
    xt, yt = x.y3(), y.y3()
    rt = residual.y3() if residual is not None else None
    if workspace is not None:
        check(
            _lib.lib().y3_conv2d_fwd_ws(C.byref(d), C.byref(xt), filt.data_ptr(), bias.data_ptr(), C.byref(rt) if rt is not None else None, C.byref(yt), workspace.data_ptr(),
                                        workspace.numel(), stream_ptr()),
            "y3_conv2d_fwd_ws",
        )
        return
    check(
        _lib.lib().y3_conv2d_fwd(C.byref(d), C.byref(xt), filt.data_ptr(), bias.data_ptr(), C.byref(rt) if rt is not None else None, C.byref(yt), stream_ptr()),
        "y3_conv2d_fwd",
    )


def conv_variant(x: View, y: View, k: int, stride: int, residual: bool = False, upsample2x: bool = False, algo: int = _lib.Y3_ALGO_AUTO, in_dilation: int = 0,
                 workspace_bytes: int = 0) -> str:
    """Name of the kernel variant the library's dispatcher picks for this problem (nothing is launched)."""
    d = Y3ConvDesc(dtype_code(x.buf.dtype), k, stride, _lib.Y3_ACT_NONE, int(upsample2x), algo, x.c, y.c, in_dilation)
    xt, yt = x.y3(), y.y3()
    name = C.create_string_buffer(64)
    check(_lib.lib().y3_conv2d_fwd_variant(C.byref(d), C.byref(xt), C.byref(yt), int(residual), workspace_bytes, name, 64), "y3_conv2d_fwd_variant")
    return name.value.decode()


def pack_filter_stem(w_oihw: torch.Tensor, cout: int, dtype: torch.dtype) -> torch.Tensor:
    """OIHW fp32 weights (cin <= 4, 3x3) -> the stem kernel's [cout_pad32][3][16] bank."""
    require_gpu(w_oihw, "pack_filter_stem")
    w = w_oihw.detach().to(torch.float32).contiguous()
    co, ci, k, _ = w.shape
    assert k == 3 and ci <= 4
    out = torch.empty(int(_lib.lib().y3_packed_filter_stem_elems(cout)), dtype=dtype, device=w.device)
    check(_lib.lib().y3_pack_filter_stem(w.data_ptr(), co, ci, cout, dtype_code(dtype), out.data_ptr(), stream_ptr()), "y3_pack_filter_stem")
    return out


def stem_conv(x_nchw: torch.Tensor, filt: torch.Tensor, bias: torch.Tensor, y: View, act: bool, divisor: float = 1.0):
    """First-layer 3x3 s1 conv straight from the NCHW image (u8 / f16 / bf16 / f32) into the NHWC view y."""
    require_gpu(x_nchw, "stem_conv")
    x = x_nchw.contiguous()
    n, c, h, w = x.shape
    check(_lib.lib().y3_stem_conv_fwd(x.data_ptr(), dtype_code(x.dtype), n, c, h, w, float(divisor), filt.data_ptr(), bias.data_ptr() if bias is not None else None,
                                      dtype_code(y.buf.dtype), _lib.Y3_ACT_SILU if act else _lib.Y3_ACT_NONE, _ref(y), stream_ptr()), "y3_stem_conv_fwd")


def stem_conv_stats_rows(n: int, h: int, w: int) -> int:
    return int(_lib.lib().y3_stem_conv_stats_rows(n, h, w))


def stem_conv_stats(x_nchw: torch.Tensor, filt: torch.Tensor, bias: torch.Tensor, y: View, stat_rows: torch.Tensor, capacity_rows: int, divisor: float = 1.0) -> int:
    """stem_conv without activation + one row of (sum, sum of squares) per filter and block in stat_rows (fp32): the training form of layer 0."""
    require_gpu(x_nchw, "stem_conv_stats")
    x = x_nchw.contiguous()
    n, c, h, w = x.shape
    rows = C.c_int64(0)
    check(_lib.lib().y3_stem_conv_fwd_stats(x.data_ptr(), dtype_code(x.dtype), n, c, h, w, float(divisor), filt.data_ptr(), bias.data_ptr() if bias is not None else None,
                                            dtype_code(y.buf.dtype), _lib.Y3_ACT_NONE, _ref(y), stat_rows.data_ptr(), int(capacity_rows), C.byref(rows), stream_ptr()),
          "y3_stem_conv_fwd_stats")
    return int(rows.value)


def stem_bwd_workspace(device) -> torch.Tensor:
    return torch.empty(int(_lib.lib().y3_stem_bn_bwd_wgrad_workspace_bytes()), dtype=torch.uint8, device=device)


def stem_bn_bwd_wgrad(x_nchw: torch.Tensor, u: View, dy: View, scale, shift, mean, invstd, act: int, sums: torch.Tensor, dgamma, dbeta, dw: torch.Tensor,
                      workspace: torch.Tensor, divisor: float = 1.0):
    """Layer 0 backward (no data gradient): BatchNorm + activation backward of dy and the filter gradient dw (fp32 OIHW) in one pass over
    (u, dy) after the reduction pass -- du is never written.  32 filters, <= 3 image channels."""
    require_gpu(x_nchw, "stem_bn_bwd_wgrad")
    x = x_nchw.contiguous()
    n, c, h, w = x.shape
    if dw.dtype != torch.float32 or not dw.is_contiguous() or tuple(dw.shape) != (32, c, 3, 3):
        raise TypeError("stem_bn_bwd_wgrad: dw must be a contiguous fp32 (32, cin, 3, 3) tensor")
    check(_lib.lib().y3_stem_bn_bwd_wgrad(x.data_ptr(), dtype_code(x.dtype), n, c, h, w, float(divisor), _ref(u), _ref(dy), scale.data_ptr(), shift.data_ptr(),
                                          mean.data_ptr(), invstd.data_ptr(), dtype_code(u.buf.dtype), int(act), sums.data_ptr(),
                                          dgamma.data_ptr() if dgamma is not None else None, dbeta.data_ptr() if dbeta is not None else None, dw.data_ptr(),
                                          workspace.data_ptr(), workspace.numel(), stream_ptr()), "y3_stem_bn_bwd_wgrad")


def pack_filter_dgrad(w_oihw: torch.Tensor, cout: int, cin: int, dtype: torch.dtype) -> torch.Tensor:
    """OIHW fp32 weights -> filter bank of the data-gradient conv (cin filters over (kh, kw, cout), flipped taps)."""
    require_gpu(w_oihw, "pack_filter_dgrad")
    w = w_oihw.detach().to(torch.float32).contiguous()
    co, ci, k, _ = w.shape
    out = torch.empty(packed_filter_elems(cin, cout, k), dtype=dtype, device=w.device)
    check(_lib.lib().y3_pack_filter_dgrad(w.data_ptr(), co, ci, k, cout, cin, dtype_code(dtype), out.data_ptr(), stream_ptr()), "y3_pack_filter_dgrad")
    return out


def bneck_pair(x: View, filt1: torch.Tensor, bias1: torch.Tensor, act1: bool, filt2: torch.Tensor, bias2: torch.Tensor, act2: bool, add: bool, y: View):
    """Bottleneck(C, C), C = 64 or 128: y = [x +] cv2(cv1(x)), cv1 1x1 C -> C/2, cv2 3x3 C/2 -> C, the intermediate kept in LDS (csrc/stem.hip)."""
    check(_lib.lib().y3_bneck_pair_fwd(_ref(x), filt1.data_ptr(), bias1.data_ptr(), _lib.Y3_ACT_SILU if act1 else _lib.Y3_ACT_NONE, filt2.data_ptr(), bias2.data_ptr(),
                                       _lib.Y3_ACT_SILU if act2 else _lib.Y3_ACT_NONE, int(bool(add)), dtype_code(x.buf.dtype), _ref(y), stream_ptr()), "y3_bneck_pair_fwd")


def last_conv_variant() -> str:
    """variant name of the last conv / data-gradient launch of this thread (tests)"""
    buf = C.create_string_buffer(64)
    check(_lib.lib().y3_conv_last_variant(buf, 64), "y3_conv_last_variant")
    return buf.value.decode()


def conv2d_dgrad_s2(w_oihw: torch.Tensor, du: View, gx: View, accumulate: bool):
    """Data gradient of a 3x3 stride-2 conv through the four output-parity class convolutions (f16/bf16)."""
    dt = du.buf.dtype
    L = _lib.lib()
    w = w_oihw.detach().to(torch.float32).contiguous()
    co, ci, k, _ = w.shape
    assert k == 3
    packed = torch.empty(int(L.y3_packed_filter_dgrad_s2_elems(du.c, gx.c)), dtype=dt, device=w.device)
    check(L.y3_pack_filter_dgrad_s2(w.data_ptr(), co, ci, du.c, gx.c, dtype_code(dt), packed.data_ptr(), stream_ptr()), "y3_pack_filter_dgrad_s2")
    dut, gxt = du.y3(), gx.y3()
    check(L.y3_conv2d_dgrad_s2(dtype_code(dt), C.byref(dut), packed.data_ptr(), C.byref(gxt) if accumulate else None, C.byref(gxt), stream_ptr()), "y3_conv2d_dgrad_s2")


def conv2d_wgrad_workspace_bytes(x: View, cout: int, k: int, stride: int) -> int:
    d = Y3ConvDesc(dtype_code(x.buf.dtype), k, stride, 0, 0, 0, x.c, cout, 0)
    xt = x.y3()
    return int(_lib.lib().y3_conv2d_wgrad_workspace_bytes(C.byref(d), C.byref(xt)))


def conv2d_wgrad(x: View, du: View, k: int, stride: int, cout_real: int, cin_real: int, want_bias: bool = False, alloc=None, workspace=None):
    """Filter gradient (cout_real, cin_real, k, k) fp32 (+ bias gradient) of a conv with input x and output-gradient du.
    `alloc(shape)` supplies the output tensors (the training plan's per-backward gradient arena); default torch.empty.  `workspace`: a caller-owned uint8 buffer
    for the split-K slabs (the training slot keeps one for all its layers: launches of one stream use it in order); default a fresh allocation per call."""
    d = Y3ConvDesc(dtype_code(x.buf.dtype), k, stride, 0, 0, 0, x.c, du.c, 0)
    if alloc is None:
        def alloc(shape):
            return torch.empty(shape, dtype=torch.float32, device=x.buf.device)
    dw = alloc((cout_real, cin_real, k, k))
    db = alloc((cout_real,)) if want_bias else None
    xt, dt = x.y3(), du.y3()
    need = int(_lib.lib().y3_conv2d_wgrad_workspace_bytes(C.byref(d), C.byref(xt)))
    ws = workspace if workspace is not None and workspace.numel() >= need else torch.empty(need, dtype=torch.uint8, device=x.buf.device)
    check(_lib.lib().y3_conv2d_wgrad(C.byref(d), C.byref(xt), C.byref(dt), cout_real, cin_real, dw.data_ptr(), db.data_ptr() if db is not None else None,
                                     ws.data_ptr(), need, stream_ptr()),
          "y3_conv2d_wgrad")
    return dw, db


def conv2d_wgrad_plan(x: View, cout: int, k: int, stride: int):
    """(tile edge, pixel slices, xcd-grouped) of the filter-gradient launch for this shape with pitch == c gradients, no channel padding and no bias gradient
    (y3_conv2d_wgrad_plan: dry run)"""
    d = Y3ConvDesc(dtype_code(x.buf.dtype), k, stride, 0, 0, 0, x.c, cout, 0)
    xt = x.y3()
    tile, slices, xg = C.c_int32(0), C.c_int64(0), C.c_int32(0)
    check(_lib.lib().y3_conv2d_wgrad_plan(C.byref(d), C.byref(xt), C.byref(tile), C.byref(slices), C.byref(xg)), "y3_conv2d_wgrad_plan")
    return int(tile.value), int(slices.value), int(xg.value)


def conv2d_wgrad_last_plan():
    """(tile edge, pixel slices, xcd-grouped) of the last conv2d_wgrad launch of this thread (y3_conv2d_wgrad_last_plan): the form that ran, not a re-derivation (tests)"""
    tile, slices, xg = C.c_int32(0), C.c_int64(0), C.c_int32(0)
    check(_lib.lib().y3_conv2d_wgrad_last_plan(C.byref(tile), C.byref(slices), C.byref(xg)), "y3_conv2d_wgrad_last_plan")
    return int(tile.value), int(slices.value), int(xg.value)


BN_PARTIAL_ROWS = 512


def bn_scratch(c: int, device) -> torch.Tensor:
    """fp64 scratch for y3_bn_stats / y3_bn_act_bwd: totals + per-block partial rows (Y3_BN_SCRATCH_DOUBLES)."""
    return torch.zeros((1 + BN_PARTIAL_ROWS) * 2 * c, dtype=torch.float64, device=device)


class BnVecs(NamedTuple):
    """the five per-layer device vectors of the BatchNorm calls: fp32 (C,) scale, shift, mean, invstd and the fp64 scratch bn_scratch (bn_act_fwd reads the first two alone)"""
    scale: torch.Tensor
    shift: torch.Tensor
    mean: torch.Tensor | None = None
    invstd: torch.Tensor | None = None
    sums: torch.Tensor | None = None

    @classmethod
    def alloc(cls, c: int, device) -> "BnVecs":
        return cls(*(torch.empty(c, dtype=torch.float32, device=device) for _ in range(4)), bn_scratch(c, device))


class BnAffine(NamedTuple):
    """what a finalize call reads of its nn.BatchNorm2d: device fp32 gamma / beta, eps, momentum, the running statistics it updates in place (None: not tracked)"""
    gamma: torch.Tensor
    beta: torch.Tensor
    eps: float = 1e-3       # (the reference's values: models/common.py:75)
    momentum: float = 0.03
    running_mean: torch.Tensor | None = None
    running_var: torch.Tensor | None = None


def bn_affine(bn, *explicit) -> BnAffine:
    """bn_affine(module): the BnAffine of an nn.BatchNorm2d; bn_affine(gamma, beta[, eps, momentum, running_mean, running_var]): of explicit tensors (tests)"""
    if isinstance(bn, torch.Tensor):
        return BnAffine(bn, *explicit)
    return BnAffine(bn.weight, bn.bias, float(bn.eps), float(bn.momentum), bn.running_mean, bn.running_var)


def _finalize_tail(a: BnAffine, v: BnVecs):
    """the eleven trailing arguments of y3_bn_finalize, y3_bn_stats_finalize, y3_bn_finalize_rows and y3_bn_finalize_devcount"""
    assert v.sums is not None, "a BatchNorm finalize call needs all five BnVecs vectors, not the (scale, shift) pair of bn_act_fwd"
    return (a.gamma.data_ptr(), a.beta.data_ptr(), a.eps, a.momentum, _ptr(a.running_mean), _ptr(a.running_var), v.scale.data_ptr(), v.shift.data_ptr(), v.mean.data_ptr(),
            v.invstd.data_ptr(), stream_ptr())


def _bwd_head(u: View, dy: View, v: BnVecs, act: int):
    """the nine leading arguments every y3_bn_act_bwd* entry point shares"""
    assert v.sums is not None, "a BatchNorm backward call needs all five BnVecs vectors, not the (scale, shift) pair of bn_act_fwd"
    return (_ref(u), _ref(dy), v.scale.data_ptr(), v.shift.data_ptr(), v.mean.data_ptr(), v.invstd.data_ptr(), dtype_code(u.buf.dtype), int(act), v.sums.data_ptr())


def bn_stats(u: View, sums: torch.Tensor):
    """sums[0 .. 2C) = per-channel (sum, sum of squares) of u"""
    check(_lib.lib().y3_bn_stats(_ref(u), dtype_code(u.buf.dtype), sums.data_ptr(), stream_ptr()), "y3_bn_stats")


def bn_stats_finalize(u: View, affine: BnAffine, v: BnVecs):
    """scale / shift / mean / invstd of v (and the running statistics) from the batch statistics of u"""
    check(_lib.lib().y3_bn_stats_finalize(_ref(u), dtype_code(u.buf.dtype), v.sums.data_ptr(), *_finalize_tail(affine, v)), "y3_bn_stats_finalize")


def bn_finalize_rows(rows: torch.Tensor, n_rows: int, count: int, c: int, affine: BnAffine, v: BnVecs):
    """the same from the `n_rows` statistics rows a conv epilogue wrote (conv2d_stats, stem_conv_stats, conv1x1_bnin_stats)"""
    check(_lib.lib().y3_bn_finalize_rows(rows.data_ptr(), int(n_rows), int(count), int(c), v.sums.data_ptr(), *_finalize_tail(affine, v)), "y3_bn_finalize_rows")


def bn_sum_rows(rows: torch.Tensor, n_rows: int, c: int, sums: torch.Tensor):
    """sums[0 .. 2C) = the column sums of the statistics rows (SyncBatchNorm: what a rank contributes to the all-reduce)"""
    check(_lib.lib().y3_bn_sum_rows(rows.data_ptr(), int(n_rows), int(c), sums.data_ptr(), stream_ptr()), "y3_bn_sum_rows")


def bn_finalize_devcount(count_dev: torch.Tensor, c: int, affine: BnAffine, v: BnVecs):
    """the same from the totals in v.sums[0 .. 2C) and an element count in device memory (fp64: both all-reduced over a SyncBatchNorm group)"""
    check(_lib.lib().y3_bn_finalize_devcount(v.sums.data_ptr(), count_dev.data_ptr(), int(c), *_finalize_tail(affine, v)), "y3_bn_finalize_devcount")


def bn_act_fwd(u: View, v: BnVecs, act: int, y: View, residual: View | None = None):
    """y = act(scale u + shift) (+ residual)"""
    check(_lib.lib().y3_bn_act_fwd(_ref(u), v.scale.data_ptr(), v.shift.data_ptr(), _ref(residual), _ref(y), dtype_code(u.buf.dtype), int(act), stream_ptr()), "y3_bn_act_fwd")


def bn_act_bwd(u: View, dy: View, v: BnVecs, act: int, du: View, dgamma, dbeta, gres: View | None = None, gres_accumulate: bool = False):
    """du, dgamma, dbeta of y = act(bn(u)) (+ residual); with `gres` the residual's gradient is written (or accumulated) on the pass that reads dy anyway"""
    head = _bwd_head(u, dy, v, act)
    if gres is None:
        check(_lib.lib().y3_bn_act_bwd(*head, _ref(du), _ptr(dgamma), _ptr(dbeta), stream_ptr()), "y3_bn_act_bwd")
    else:
        check(_lib.lib().y3_bn_act_bwd_res(*head, _ref(du), _ptr(dgamma), _ptr(dbeta), _ref(gres), int(bool(gres_accumulate)), stream_ptr()), "y3_bn_act_bwd_res")


def bn_act_bwd_reduce(u: View, dy: View, v: BnVecs, act: int, dgamma, dbeta):
    """first half of bn_act_bwd: this rank's reduction totals into v.sums[0 .. 2C), dgamma, dbeta (SyncBatchNorm all-reduces the totals before the second half)"""
    check(_lib.lib().y3_bn_act_bwd_reduce(*_bwd_head(u, dy, v, act), _ptr(dgamma), _ptr(dbeta), stream_ptr()), "y3_bn_act_bwd_reduce")


def bn_act_bwd_apply(u: View, dy: View, v: BnVecs, act: int, du: View, gres: View | None = None, gres_accumulate: bool = False):
    """second half of bn_act_bwd: du (and the residual's gradient) from the means in v.sums[2C .. 4C)"""
    check(_lib.lib().y3_bn_act_bwd_apply(*_bwd_head(u, dy, v, act), _ref(du), _ref(gres), int(bool(gres_accumulate)), stream_ptr()), "y3_bn_act_bwd_apply")


def nchw_to_nhwc(src: torch.Tensor, out: View, divisor: float = 1.0):
    require_gpu(src, "nchw_to_nhwc")
    src = src.contiguous()
    n, c, h, w = src.shape
    check(_lib.lib().y3_nchw_to_nhwc(src.data_ptr(), dtype_code(src.dtype), n, c, h, w, float(divisor), dtype_code(out.buf.dtype), _ref(out), stream_ptr()), "y3_nchw_to_nhwc")


def nhwc_to_nchw(src: View) -> torch.Tensor:
    dst = torch.empty(src.n, src.c, src.h, src.w, dtype=src.buf.dtype, device=src.buf.device)
    check(_lib.lib().y3_nhwc_to_nchw(_ref(src), dtype_code(src.buf.dtype), dst.data_ptr(), stream_ptr()), "y3_nhwc_to_nchw")
    return dst


def maxpool2d(x: View, y: View, k: int, stride: int, pad: int, zpad_r: int = 0, zpad_b: int = 0):
    check(_lib.lib().y3_maxpool2d(_ref(x), _ref(y), dtype_code(x.buf.dtype), k, stride, pad, zpad_r, zpad_b, stream_ptr()), "y3_maxpool2d")


def maxpool2d_bwd(x: View, dy: View, dx: View, k: int, stride: int, pad: int, zpad_r: int = 0, zpad_b: int = 0, accumulate: bool = False):
    """dx (+)= backward of MaxPool2d(k, stride, pad) (+ right / bottom zero pad) through the indexed two-pass form (a byte of scratch per output element)"""
    xt, gt, dt = x.y3(), dy.y3(), dx.y3()
    need = int(_lib.lib().y3_maxpool2d_bwd_workspace_bytes(C.byref(xt), k, stride, pad, zpad_r, zpad_b))
    ws = torch.empty(max(need, 1), dtype=torch.uint8, device=x.buf.device)
    check(_lib.lib().y3_maxpool2d_bwd_ws(C.byref(xt), C.byref(gt), C.byref(dt), dtype_code(x.buf.dtype), k, stride, pad, zpad_r, zpad_b, int(bool(accumulate)), ws.data_ptr(), need,
                                         stream_ptr()), "y3_maxpool2d_bwd_ws")


def maxpool2d_bwd_gather(x: View, dy: View, dx: View, k: int, stride: int, pad: int, zpad_r: int = 0, zpad_b: int = 0, accumulate: bool = False):
    """maxpool2d_bwd through the one-pass gather form (k^2 windows of k^2 elements per input element: the training plans run the indexed form; tests compare the two)"""
    check(_lib.lib().y3_maxpool2d_bwd(_ref(x), _ref(dy), _ref(dx), dtype_code(x.buf.dtype), k, stride, pad, zpad_r, zpad_b, int(bool(accumulate)), stream_ptr()), "y3_maxpool2d_bwd")


def spp_pyramid(x: View, y3c: View):
    check(_lib.lib().y3_spp_pyramid(_ref(x), _ref(y3c), dtype_code(x.buf.dtype), stream_ptr()), "y3_spp_pyramid")


def upsample2x(x: View, y: View):
    check(_lib.lib().y3_upsample2x(_ref(x), _ref(y), dtype_code(x.buf.dtype), stream_ptr()), "y3_upsample2x")


def upsample2x_bwd(dy: View, dx: View, accumulate: bool):
    check(_lib.lib().y3_upsample2x_bwd(_ref(dy), _ref(dx), dtype_code(dy.buf.dtype), int(bool(accumulate)), stream_ptr()), "y3_upsample2x_bwd")


def copy_slice(x: View, y: View):
    check(_lib.lib().y3_copy_slice(_ref(x), _ref(y), dtype_code(x.buf.dtype), stream_ptr()), "y3_copy_slice")


def detect_decode(head: View, na: int, no: int, anchors_px, stride: float, raw: torch.Tensor | None, z: torch.Tensor | None, row_offset: int, total_rows: int):
    arr = (C.c_float * (na * 2))(*[float(v) for v in anchors_px])
    check(
        _lib.lib().y3_detect_decode(
            _ref(head), dtype_code(head.buf.dtype), na, no, arr, float(stride), raw.data_ptr() if raw is not None else None, z.data_ptr() if z is not None else None,
            row_offset, total_rows, stream_ptr(),
        ),
        "y3_detect_decode",
    )


def detect_decode_levels(heads, na: int, no: int, anchors_px, strides, raws, z: torch.Tensor | None, row_offsets, total_rows: int) -> bool:
    """every level of a Detect head in ONE launch (y3_detect_decode_levels: the tiled kernel of the 2-byte dtypes).  heads: Views; anchors_px: per level na * 2 floats;
    raws: per level a tensor or None (or None for none at all).  False = the library refused (a level is not eligible for that kernel, or knob decode_tile = 0) and
    launched nothing: call detect_decode per level -- the same values, bit for bit."""
    nl = len(heads)
    ts = (_lib.Y3Tensor * nl)(*[h.y3() for h in heads])
    anc = (C.c_float * (nl * na * 2))(*[float(v) for a in anchors_px for v in a])
    st = (C.c_float * nl)(*[float(s) for s in strides])
    rp = (C.c_void_p * nl)(*[r.data_ptr() if r is not None else None for r in (raws if raws is not None else [None] * nl)])
    ro = (C.c_int64 * nl)(*[int(r) for r in row_offsets])
    return _lib.lib().y3_detect_decode_levels(ts, nl, dtype_code(heads[0].buf.dtype), na, no, anc, st, rp, z.data_ptr() if z is not None else None, ro, total_rows, stream_ptr()) == 0


def detect_raw_bwd(graw: torch.Tensor, na: int, no: int, ghead: View):
    """ghead[b, y, x, a * no + o] = graw[b, a, y, x, o] (contiguous, ghead's dtype); the pad channels of ghead are zeroed"""
    check(_lib.lib().y3_detect_raw_bwd(graw.data_ptr(), dtype_code(graw.dtype), ghead.n, na, ghead.h, ghead.w, no, _ref(ghead), stream_ptr()), "y3_detect_raw_bwd")


_nms_ws_cache: dict = {}


def nms_raw(pred: torch.Tensor, conf_thres: float, iou_thres: float, classes, agnostic: bool, multi_label: bool, max_det: int, max_nms: int = 30000,
            max_wh: float = 7680.0):
    """Batched NMS on device.  Returns (rows (bs,max_det,6) fp32, counts list[int]).  One D2H copy (counts+status)."""
    require_gpu(pred, "non_max_suppression")
    pred = pred.contiguous()
    bs, n_rows, no = pred.shape
    nc = no - 5
    dev = pred.device
    cls_t = torch.tensor(list(classes), dtype=torch.int32, device=dev) if classes is not None else None
    p = Y3NmsParams(float(iou_thres), float(conf_thres), int(bool(multi_label)), int(bool(agnostic)), int(max_det), int(max_nms), float(max_wh),
                    0 if cls_t is None else cls_t.numel())
    L = _lib.lib()
    rows = torch.empty(bs, max_det, 6, dtype=torch.float32, device=dev)
    meta = torch.empty(bs + 2, dtype=torch.int32, device=dev)
    capacity = 0
    for attempt in range(3):
        need = int(L.y3_nms_workspace_bytes(bs, n_rows, nc, C.byref(p), capacity))
        key = (dev.index, need)
        ws = _nms_ws_cache.get(key)
        if ws is None:
            ws = torch.empty(need, dtype=torch.uint8, device=dev)
            if need <= (1 << 30):
                _nms_ws_cache[key] = ws
        check(
            L.y3_nms(pred.data_ptr(), dtype_code(pred.dtype), bs, n_rows, nc, C.byref(p), cls_t.data_ptr() if cls_t is not None else None, rows.data_ptr(),
                     meta.data_ptr(), meta.data_ptr() + bs * 4, capacity, ws.data_ptr(), need, stream_ptr()),
            "y3_nms",
        )
        m = meta.tolist()  # the single device->host sync of the call
        nms_raw.last_candidates = m[bs + 1]   # candidates (rows above conf_thres, one per class under multi_label) of the whole batch: bench.py reports it
        nms_raw.last_round2 = m[bs] >> 1     # images that took the second round (knob nms_head): above the overflow bit of the status word
        if (m[bs] & 1) == 0:
            return rows, m[:bs]
        capacity = max(m[bs + 1], 1)  # overflow: rerun with room for every candidate
    raise _lib.Y3Error("y3_nms: candidate capacity overflow persisted")


def scale_boxes_raw(rows: torch.Tensor, img_stride: int, row_stride: int, counts: torch.Tensor | None, bs: int, max_rows: int, params: torch.Tensor):
    require_gpu(rows, "scale_boxes")
    check(_lib.lib().y3_scale_boxes(rows.data_ptr(), int(img_stride), int(row_stride), counts.data_ptr() if counts is not None else None, int(bs), int(max_rows),
                                    params.data_ptr(), stream_ptr()), "y3_scale_boxes")


def match_detections_raw(dets: torch.Tensor, img_stride: int, row_stride: int, counts: torch.Tensor | None, bs: int, max_det: int, labels: torch.Tensor,
                         offsets: torch.Tensor, iouv: torch.Tensor) -> torch.Tensor:
    require_gpu(dets, "process_batch")
    correct = torch.empty(bs, max_det, iouv.numel(), dtype=torch.uint8, device=dets.device)
    check(_lib.lib().y3_match_detections(dets.data_ptr(), int(img_stride), int(row_stride), counts.data_ptr() if counts is not None else None, int(bs), int(max_det),
                                         labels.data_ptr() if labels.numel() else None, offsets.data_ptr(), iouv.data_ptr(), int(iouv.numel()), correct.data_ptr(), stream_ptr()),
          "y3_match_detections")
    return correct


def val_stats_append(conf: torch.Tensor, cls: torch.Tensor, img_stride: int, elem_stride: int, counts: torch.Tensor | None, bs: int, max_det: int, correct: torch.Tensor,
                     dst_conf: torch.Tensor, dst_cls: torch.Tensor, dst_mask: torch.Tensor, dst_offset: int):
    """rows of one batch behind `dst_offset` of the run's dense buffers (y3_val_stats_append); conf / cls are fp32 views whose data_ptr is the first row's element"""
    require_gpu(conf, "ValStats")
    require_gpu(correct, "ValStats")
    if conf.dtype != torch.float32 or cls.dtype != torch.float32 or correct.dtype not in (torch.uint8, torch.bool) or not correct.is_contiguous():
        raise TypeError("val_stats_append expects fp32 confidences / classes and a contiguous uint8 / bool (rows, T) hit matrix")
    check(_lib.lib().y3_val_stats_append(conf.data_ptr(), cls.data_ptr(), int(img_stride), int(elem_stride), counts.data_ptr() if counts is not None else None, int(bs), int(max_det),
                                         correct.data_ptr(), int(correct.shape[-1]), dst_conf.data_ptr(), dst_cls.data_ptr(), dst_mask.data_ptr(), int(dst_offset),
                                         int(dst_conf.numel()), stream_ptr()), "y3_val_stats_append")


def val_stats_count_labels(cls: torch.Tensor, stride: int, n: int, nt: torch.Tensor):
    if n:
        require_gpu(cls, "ValStats")
    check(_lib.lib().y3_val_stats_count_labels(cls.data_ptr() if n else None, int(stride), int(n), nt.data_ptr(), int(nt.numel()), stream_ptr()), "y3_val_stats_count_labels")


_val_stats_cache: dict = {}


def val_stats_compute(conf: torch.Tensor, cls: torch.Tensor, mask: torch.Tensor, n: int, nt: torch.Tensor, niou: int, eps: float) -> torch.Tensor:
    """ap_per_class for the first n rows of the run's buffers (y3_val_stats_compute) -> the DEVICE result block (fp64), see include/yolov3_hip.h"""
    require_gpu(nt, "ValStats")
    import numpy as np

    dev, nc, L = nt.device, int(nt.numel()), _lib.lib()
    grids = _val_stats_cache.get(("grids", dev.index))
    if grids is None:   # np.linspace's own values: the sample points of the reference
        grids = _val_stats_cache[("grids", dev.index)] = (torch.from_numpy(np.linspace(0.0, 1.0, 1000)).to(dev), torch.from_numpy(np.linspace(0.0, 1.0, 101)).to(dev))
    need = int(L.y3_val_stats_workspace_bytes(int(n), nc))
    if need == 0:
        check(-1, "y3_val_stats_workspace_bytes")
    ws = _val_stats_cache.get(("ws", dev.index))
    if ws is None or ws.numel() < need:
        ws = _val_stats_cache[("ws", dev.index)] = torch.empty(need, dtype=torch.uint8, device=dev)
    out = torch.empty(int(L.y3_val_stats_out_elems(nc, int(niou))), dtype=torch.float64, device=dev)
    check(L.y3_val_stats_compute(conf.data_ptr() if n else None, cls.data_ptr() if n else None, mask.data_ptr() if n else None, int(n), nt.data_ptr(), nc, int(niou), float(eps),
                                 grids[0].data_ptr(), grids[1].data_ptr(), out.data_ptr(), out.numel(), ws.data_ptr(), ws.numel(), stream_ptr()), "y3_val_stats_compute")
    return out


def confusion_matrix_raw(dets: torch.Tensor | None, img_stride: int, row_stride: int, counts: torch.Tensor | None, bs: int, max_det: int, labels: torch.Tensor, label_stride: int,
                         offsets: torch.Tensor, nc: int, conf: float, iou_thres: float, matrix: torch.Tensor):
    require_gpu(matrix, "ConfusionMatrix")
    check(_lib.lib().y3_confusion_matrix(dets.data_ptr() if dets is not None else None, int(img_stride), int(row_stride), counts.data_ptr() if counts is not None else None, int(bs),
                                         int(max_det), labels.data_ptr() if labels.numel() else None, int(label_stride), offsets.data_ptr(), int(nc), float(conf), float(iou_thres),
                                         matrix.data_ptr(), stream_ptr()), "y3_confusion_matrix")


def labels_to_native(targets: torch.Tensor, bs: int, width: int, height: int, params: torch.Tensor):
    """collate-format targets (nl, 6) on the device -> (labels (nl, 5) native pixels, offsets (bs + 1) int32), y3_labels_to_native"""
    require_gpu(targets, "labels_to_native")
    if targets.dtype != torch.float32 or targets.dim() != 2 or targets.shape[1] != 6 or not targets.is_contiguous():
        raise TypeError("labels_to_native expects contiguous fp32 (nl, 6) targets [image, class, x, y, w, h]")
    nl = targets.shape[0]
    out = torch.empty(nl, 5, dtype=torch.float32, device=targets.device)
    offs = torch.empty(bs + 1, dtype=torch.int32, device=targets.device)
    check(_lib.lib().y3_labels_to_native(targets.data_ptr() if nl else None, nl, int(bs), float(width), float(height), params.data_ptr(), out.data_ptr() if nl else None,
                                         offs.data_ptr(), stream_ptr()), "y3_labels_to_native")
    return out, offs


def label_rows(pred: torch.Tensor, row0: int, n_rows: int, targets: torch.Tensor, offsets: torch.Tensor, width: float = 1.0, height: float = 1.0):
    """rows [row0, row0 + n_rows) of every image of the contiguous (bs, rows, no) prediction become the a-priori label rows of non_max_suppression(labels=...):
    targets (nl, 6) fp32 [image, class, x, y, w, h] on the device, grouped by image through offsets (bs + 1 int32); xywh * (width, height, width, height), objectness 1,
    one-hot class, zero rows past an image's labels (y3_label_rows).  In place; the rows outside the window are not touched."""
    require_gpu(pred, "label_rows")
    if pred.dim() != 3 or not pred.is_contiguous():
        raise TypeError("label_rows expects a contiguous (bs, rows, no) prediction")
    bs, total, no = pred.shape
    if targets.dtype != torch.float32 or targets.dim() != 2 or targets.shape[1] != 6 or not targets.is_contiguous() or targets.device != pred.device:
        raise TypeError("label_rows expects contiguous fp32 (nl, 6) targets [image, class, x, y, w, h] on the prediction's device")
    if offsets.dtype != torch.int32 or offsets.numel() != bs + 1 or not offsets.is_contiguous() or offsets.device != pred.device:
        raise TypeError("label_rows expects bs + 1 int32 label offsets on the prediction's device")
    if row0 < 0 or n_rows < 0 or row0 + n_rows > total:
        raise ValueError(f"label_rows: rows [{row0}, {row0 + n_rows}) do not fit a prediction of {total} rows")
    nl = targets.shape[0]
    check(_lib.lib().y3_label_rows(targets.data_ptr() if nl else None, nl, offsets.data_ptr(), bs, float(width), float(height), pred.data_ptr(), dtype_code(pred.dtype), total, no,
                                   int(row0), int(n_rows), stream_ptr()), "y3_label_rows")


EXPORT_FORMS = {"target": _lib.Y3_EXPORT_TARGET, "txt": _lib.Y3_EXPORT_TXT, "json": _lib.Y3_EXPORT_JSON}


def export_rows(rows: torch.Tensor, img_stride: int, row_stride: int, counts: torch.Tensor | None, bs: int, max_rows: int, form: str, total: int, limit: int = 0,
                round_boxes: bool = False, reverse: bool = False, image0: int = 0, sizes: torch.Tensor | None = None, nc: int = 0):
    """The padded NMS result (as scale_boxes_raw takes it) -> (table (total, 7) fp32, offsets (bs + 1) int32, class_counts (bs, nc) int32 or None), all on the device, in one
    launch (y3_export_rows).  `form`: "target" [image, cls, cx, cy, w, h, conf], "txt" (xywh / native size; `sizes` (bs, 2) fp32 {w0, h0} on the device) or "json" (top-left corner).
    `total`: the rows the caller expects, i.e. sum(min(count, max_rows, limit)) from the counts NMS already brought to the host; rows beyond it are dropped.  `nc` > 0 also
    returns the per-image histogram of the class column."""
    require_gpu(rows, "export_rows")
    if rows.dtype != torch.float32:
        raise TypeError("export_rows expects fp32 rows [x1, y1, x2, y2, conf, cls]")
    if form not in EXPORT_FORMS:
        raise ValueError(f"export_rows: form {form!r} is not one of {sorted(EXPORT_FORMS)}")
    dev = rows.device
    if counts is not None and (counts.dtype != torch.int32 or counts.device != dev or counts.numel() != bs or not counts.is_contiguous()):
        raise TypeError("export_rows expects bs int32 counts on the rows' device")
    if sizes is not None and (sizes.dtype != torch.float32 or sizes.device != dev or sizes.numel() != 2 * bs or not sizes.is_contiguous()):
        raise TypeError("export_rows expects (bs, 2) fp32 native sizes {w0, h0} on the rows' device")
    table = torch.empty(int(total), 7, dtype=torch.float32, device=dev)
    offsets = torch.empty(bs + 1, dtype=torch.int32, device=dev)
    hist = torch.zeros(bs, nc, dtype=torch.int32, device=dev) if nc > 0 else None   # (the export adds into it)
    check(_lib.lib().y3_export_rows(rows.data_ptr(), int(img_stride), int(row_stride), _ptr(counts), int(bs), int(max_rows), EXPORT_FORMS[form], int(limit), int(bool(round_boxes)),
                                    int(bool(reverse)), int(image0), _ptr(sizes), table.data_ptr() if total else None, int(total), offsets.data_ptr(), _ptr(hist), int(nc), stream_ptr()),
          "y3_export_rows")
    return table, offsets, hist


def scale_img(img: torch.Tensor, ratio: float = 1.0, same_shape: bool = False, gs: int = 32, flip_lr: bool = False) -> torch.Tensor:
    """upstream scale_img (the resize + pad of reference models/yolo.py:246), fused with the left-right mirror of the same line: (n, c, h, w) ->
    (n, c, ceil(h ratio / gs) gs, ceil(w ratio / gs) gs).  ratio 1.0 without a mirror returns `img` itself, like upstream."""
    if ratio == 1.0 and not flip_lr:
        return img
    require_gpu(img, "scale_img")
    if img.dim() != 4 or img.dtype not in (torch.float32, torch.float16, torch.bfloat16):
        raise TypeError("scale_img expects a floating (n, c, h, w) batch")
    img = img.contiguous()
    n, c, h, w = img.shape
    ih, iw = (h, w) if ratio == 1.0 else (int(h * ratio), int(w * ratio))
    oh, ow = (ih, iw) if (same_shape or ratio == 1.0) else (math.ceil(h * ratio / gs) * gs, math.ceil(w * ratio / gs) * gs)
    out = torch.empty(n, c, oh, ow, dtype=img.dtype, device=img.device)
    check(_lib.lib().y3_scale_img(img.data_ptr(), dtype_code(img.dtype), n, c, h, w, ih, iw, oh, ow, int(bool(flip_lr)), 0.447, out.data_ptr(), stream_ptr()), "y3_scale_img")
    return out


def resize_bilinear(x: torch.Tensor, size, out_dtype: torch.dtype | None = None, div: float = 1.0) -> torch.Tensor:
    """F.interpolate(x.float() / div, size=size, mode="bilinear", align_corners=False) rounded once to out_dtype, in one launch (reference train.py:380 + 399):
    (n, c, h, w) uint8 / float32 / float16 / bfloat16 -> (n, c, size[0], size[1]) in out_dtype (default: x's dtype, float32 for uint8)."""
    require_gpu(x, "resize_bilinear")
    if x.dim() != 4 or x.dtype not in (torch.uint8, torch.float32, torch.float16, torch.bfloat16):
        raise TypeError("resize_bilinear expects a uint8 or floating (n, c, h, w) batch")
    if out_dtype is None:
        out_dtype = torch.float32 if x.dtype == torch.uint8 else x.dtype
    if out_dtype not in (torch.float32, torch.float16, torch.bfloat16):
        raise TypeError(f"resize_bilinear writes float32 / float16 / bfloat16, not {out_dtype}")
    oh, ow = (int(s) for s in size)
    x = x.contiguous()
    n, c, h, w = x.shape
    out = torch.empty(n, c, oh, ow, dtype=out_dtype, device=x.device)
    if n == 0:   # (an empty tensor has no address to hand over)
        return out
    check(_lib.lib().y3_resize_bilinear(x.data_ptr(), dtype_code(x.dtype), n, c, h, w, out.data_ptr(), dtype_code(out_dtype), oh, ow, float(div), stream_ptr()), "y3_resize_bilinear")
    return out


def quad_collate_u8(x: torch.Tensor, flags: torch.Tensor) -> torch.Tensor:
    """The image half of the reference's collate_fn4 (utils/dataloaders.py:842-853) in one launch: uint8 (bs, c, h, w), bs % 4 == 0, and bs / 4 uint8 flags on the
    device -> uint8 (bs / 4, c, 2h, 2w); group g is the bilinear x2 upsample of image 4g where flags[g] is set, the 2x2 tile of images 4g .. 4g+3 otherwise."""
    require_gpu(x, "quad_collate_u8")
    require_gpu(flags, "quad_collate_u8")
    if x.dim() != 4 or x.dtype != torch.uint8:
        raise TypeError("quad_collate_u8 expects a uint8 (bs, c, h, w) batch")
    bs, c, h, w = x.shape
    if bs % 4:
        raise ValueError(f"quad_collate_u8: batch size {bs} is not a multiple of 4")
    if flags.dtype != torch.uint8 or flags.dim() != 1 or flags.numel() != bs // 4 or flags.device != x.device:
        raise TypeError(f"quad_collate_u8 expects {bs // 4} uint8 flags on {x.device}")
    x, flags = x.contiguous(), flags.contiguous()
    out = torch.empty(bs // 4, c, 2 * h, 2 * w, dtype=torch.uint8, device=x.device)
    if bs:
        check(_lib.lib().y3_quad_collate_u8(x.data_ptr(), bs, c, h, w, flags.data_ptr(), out.data_ptr(), stream_ptr()), "y3_quad_collate_u8")
    return out


def descale_pred_into(pred: torch.Tensor, row0: int, nrows: int, scale: float, flip, img_size, out: torch.Tensor, out_row0: int):
    """rows [row0, row0 + nrows) of the decoded prediction (bs, rows, no) of one augmentation pass, de-scaled / de-mirrored (reference models/yolo.py:253-267),
    into rows [out_row0, ...) of the concatenated result."""
    require_gpu(pred, "_descale_pred")
    if pred.dim() != 3 or out.dim() != 3 or pred.dtype != out.dtype or not pred.is_contiguous() or not out.is_contiguous() or pred.shape[0] != out.shape[0] or pred.shape[2] != out.shape[2]:
        raise TypeError("descale_pred_into expects contiguous (bs, rows, no) tensors of one dtype")
    check(_lib.lib().y3_descale_pred(pred.data_ptr(), dtype_code(pred.dtype), pred.shape[0], pred.shape[1], pred.shape[2], int(row0), int(nrows), float(scale), int(flip or 0),
                                     float(img_size[0]), float(img_size[1]), out.data_ptr(), out.shape[1], int(out_row0), stream_ptr()), "y3_descale_pred")


def letterbox_u8(src_hwc: torch.Tensor, dst_batch: torch.Tensor, index: int, new_h: int, new_w: int, top: int, left: int, color: int = 114):
    """One image (h0, w0, >=3) uint8 on the device -> image `index` of the (n, 3, H1, W1) uint8 batch (resize + pad + transpose)."""
    require_gpu(src_hwc, "letterbox")
    if src_hwc.dtype != torch.uint8 or dst_batch.dtype != torch.uint8 or src_hwc.dim() != 3 or dst_batch.dim() != 4 or not src_hwc.is_contiguous() or not dst_batch.is_contiguous():
        raise TypeError("letterbox expects a contiguous (h, w, c) uint8 image and a contiguous (n, 3, H, W) uint8 batch")
    h0, w0, cs = src_hwc.shape
    check(_lib.lib().y3_letterbox_u8(src_hwc.data_ptr(), h0, w0, cs, dst_batch.data_ptr(), int(index), dst_batch.shape[2], dst_batch.shape[3], int(new_h), int(new_w), int(top),
                                     int(left), int(color), stream_ptr()), "y3_letterbox_u8")


def conv2d_stats_rows(x: View, y: View, k: int, stride: int, workspace: torch.Tensor | None = None) -> int:
    """rows of the statistics buffer a conv2d_stats launch of this shape writes (depends on the dispatched tile variant)."""
    d = Y3ConvDesc(dtype_code(x.buf.dtype), k, stride, _lib.Y3_ACT_NONE, 0, _lib.Y3_ALGO_AUTO, x.c, y.c, 0)
    xt, yt = x.y3(), y.y3()
    if workspace is not None:
        rows = int(_lib.lib().y3_conv2d_fwd_stats_rows_ws(C.byref(d), C.byref(xt), C.byref(yt), workspace.numel()))
    else:
        rows = int(_lib.lib().y3_conv2d_fwd_stats_rows(C.byref(d), C.byref(xt), C.byref(yt)))
    if rows < 0:
        check(-1, "y3_conv2d_fwd_stats_rows")
    return rows


def conv1x1_bnin_rows(u_in: View, y_in: View, y: View, has_shortcut: bool) -> int:
    """statistics rows of a conv1x1_bnin_stats launch of this shape, or -1 when the library's input-transform form (csrc/conv_1x1s.h) does not cover it"""
    d = Y3ConvDesc(dtype_code(u_in.buf.dtype), 1, 1, _lib.Y3_ACT_NONE, 0, _lib.Y3_ALGO_AUTO, u_in.c, y.c, 0)
    # geometry only (nothing is dereferenced): the views may not be bound to memory yet (TrainPlan builds before its arena exists)
    ut, it, yt = (Y3Tensor(4096, v.n, v.h, v.w, v.c, v.pitch) for v in (u_in, y_in, y))
    return int(_lib.lib().y3_conv2d_fwd_bnin_rows(C.byref(d), C.byref(ut), C.byref(it), C.byref(yt), int(bool(has_shortcut))))


def conv1x1_bnin_stats(u_in: View, in_scale: torch.Tensor, in_shift: torch.Tensor, in_act: int, shortcut: View | None, y_in: View, filt: torch.Tensor, bias: torch.Tensor, y: View,
                       stat_rows: torch.Tensor, capacity_rows: int) -> int:
    """y_in = act(in_scale * u_in + in_shift) (+ shortcut), stored once, and y = conv1x1(y_in) with statistics rows -- one launch (the producing layer's BatchNorm applied on the
    way into its 1x1 consumer: no normalise pass, no second read of y_in)."""
    d = Y3ConvDesc(dtype_code(u_in.buf.dtype), 1, 1, _lib.Y3_ACT_NONE, 0, _lib.Y3_ALGO_AUTO, u_in.c, y.c, 0, filt.numel())
    ut, it, yt = u_in.y3(), y_in.y3(), y.y3()
    st = shortcut.y3() if shortcut is not None else None
    n = C.c_int64(0)
    check(_lib.lib().y3_conv2d_fwd_bnin_stats(C.byref(d), C.byref(ut), in_scale.data_ptr(), in_shift.data_ptr(), int(in_act), C.byref(st) if st is not None else None, C.byref(it),
                                              filt.data_ptr(), bias.data_ptr(), C.byref(yt), stat_rows.data_ptr(), int(capacity_rows), C.byref(n), stream_ptr()), "y3_conv2d_fwd_bnin_stats")
    return int(n.value)


def conv2d_stats(x: View, filt: torch.Tensor, bias: torch.Tensor, y: View, k: int, stride: int, stat_rows: torch.Tensor, capacity_rows: int,
                 workspace: torch.Tensor | None = None) -> int:
    """y = conv(x) (no activation) + per-(pixel tile, wave) rows of (sum, sum of squares) per filter in stat_rows (fp32)."""
    d = Y3ConvDesc(dtype_code(x.buf.dtype), k, stride, _lib.Y3_ACT_NONE, 0, _lib.Y3_ALGO_AUTO, x.c, y.c, 0, filt.numel())
    xt, yt = x.y3(), y.y3()
    n = C.c_int64(0)
    if workspace is not None:
        check(_lib.lib().y3_conv2d_fwd_stats_ws(C.byref(d), C.byref(xt), filt.data_ptr(), bias.data_ptr(), C.byref(yt), stat_rows.data_ptr(), int(capacity_rows), C.byref(n),
                                                workspace.data_ptr(), workspace.numel(), stream_ptr()), "y3_conv2d_fwd_stats_ws")
        return int(n.value)
    check(_lib.lib().y3_conv2d_fwd_stats(C.byref(d), C.byref(xt), filt.data_ptr(), bias.data_ptr(), C.byref(yt), stat_rows.data_ptr(), int(capacity_rows), C.byref(n), stream_ptr()),
          "y3_conv2d_fwd_stats")
    return int(n.value)


def pack_job_blocks(k: int, cout: int, cin: int, want_fwd: bool = True, want_dgrad: bool = False) -> int:
    """blocks one job occupies in the grid of y3_pack_filter_jobs / y3_fold_pack_jobs: the jobs lie back to back, first_block = running sum"""
    return int(_lib.lib().y3_pack_job_blocks(k, cout, cin, int(want_fwd), int(want_dgrad)))


def job_table(records, device) -> torch.Tensor:
    """a list of ctypes records (_lib.Y3PackJob / _lib.Y3FoldPackJob) -> the device array the jobs launches read"""
    host = torch.frombuffer(bytearray(b"".join(bytes(r) for r in records)), dtype=torch.uint8)
    return host.to(device)


def fold_pack_jobs(table: torch.Tensor, n_jobs: int, blocks: int, dtype: torch.dtype):
    """Conv + BatchNorm fold and pack of every job of a device table of _lib.Y3FoldPackJob records in one launch (engine.FoldPackJobs)"""
    check(_lib.lib().y3_fold_pack_jobs(table.data_ptr(), int(n_jobs), int(blocks), dtype_code(dtype), stream_ptr()), "y3_fold_pack_jobs")


class PackJobs:
    """Every layer's filter banks in one launch (y3_pack_filter_jobs): `add` registers a layer and returns its persistent (forward bank,
    data-gradient bank) tensors, `run` re-packs them from the current fp32 weights.  The job table lives on the device and is
    rebuilt only when a weight tensor moved (data_ptr changed).

    `run(select)` packs a subset: `select` is a sequence of (job index, always).  A job with `always` (a weight that is being trained: the optimizer may have
    written it since the last forward) is packed at every call; one without (a frozen weight) is packed when its banks do not hold the tensor's current
    (data_ptr, _version) -- once, and again after load_state_dict or any other in-place write that torch's version counter sees."""

    MAX_TABLES = 8   # device job tables kept, one per distinct set of jobs packed together (all of a plan's jobs; the live ones of a frozen plan)

    def __init__(self, dtype: torch.dtype, device):
        self.dtype, self.device = dtype, device
        self.jobs = []          # (weight param, fwd bank | None, dgrad bank | None, cout, cin)
        self._packed = []       # per job: the (data_ptr, _version) of the weight its banks were packed from as a frozen job; None = unknown (never packed, or packed as a live one)
        self._tables = {}       # job indices -> (device table, the weights' data_ptrs, blocks)
        self._same_weight = {}  # id(weight) -> its jobs (plans that freeze different layers want different banks of one weight)

    def add(self, w: torch.Tensor, cout: int, cin: int, want_fwd: bool = True, want_dgrad: bool = True):
        co, ci, k, _ = w.shape
        # zero-filled ONCE: y3_pack_filter_jobs writes only the elements that come from a weight (the row / K padding of a bank stays zero)
        fwd = torch.zeros(packed_filter_elems(cout, cin, k), dtype=self.dtype, device=self.device) if want_fwd else None
        dg = torch.zeros(packed_filter_elems(cin, cout, k), dtype=self.dtype, device=self.device) if want_dgrad else None
        self.jobs.append((w, fwd, dg, cout, cin))
        self._packed.append(None)
        self._same_weight.setdefault(id(w), []).append(len(self.jobs) - 1)
        self._tables.pop(tuple(range(len(self.jobs) - 1)), None)   # ("every job" has one more member now)
        return fwd, dg

    def stale(self, select=None):
        """the job indices `run(select)` would pack now"""
        if select is None:
            return tuple(range(len(self.jobs)))
        return tuple(i for i, always in select if always or self._packed[i] is None or self._packed[i] != (self.jobs[i][0].data_ptr(), self.jobs[i][0]._version))

    def run(self, select=None):
        todo = self.stale(select)
        if not todo:
            return
        ptrs = [self.jobs[i][0].data_ptr() for i in todo]
        ent = self._tables.get(todo)
        if ent is None or ent[1] != ptrs:
            rows, first = [], 0
            for i, ptr in zip(todo, ptrs):
                w, fwd, dg, cout, cin = self.jobs[i]
                if w.dtype != torch.float32 or not w.is_contiguous():
                    raise TypeError("PackJobs expects contiguous fp32 master weights")
                co, ci, k, _ = w.shape
                rows.append(_lib.Y3PackJob(ptr, fwd.data_ptr() if fwd is not None else 0, dg.data_ptr() if dg is not None else 0, co, ci, k, cout, cin, first))
                first += pack_job_blocks(k, cout, cin, fwd is not None, dg is not None)
            table = job_table(rows, self.device)
            self._tables.pop(todo, None)
            while len(self._tables) >= self.MAX_TABLES:
                self._tables.pop(next(iter(self._tables)))
            ent = self._tables[todo] = (table, ptrs, first)
        check(_lib.lib().y3_pack_filter_jobs(ent[0].data_ptr(), len(todo), ent[2], dtype_code(self.dtype), stream_ptr()), "y3_pack_filter_jobs")
        # a weight that is being trained may be written by a kernel torch's version counter does not see (FusedSGD): nothing is remembered about ANY of its jobs, so a plan
        # that freezes it later packs it afresh
        always = {i for i, a in select if a} if select is not None else set(todo)
        for i, ptr in zip(todo, ptrs):
            if i in always:
                for j in self._same_weight.get(id(self.jobs[i][0]), (i,)):
                    self._packed[j] = None
            else:
                self._packed[i] = (ptr, self.jobs[i][0]._version)


def stem_pair(x_nchw: torch.Tensor, filt0: torch.Tensor, bias0: torch.Tensor, act0: bool, filt1: torch.Tensor, bias1: torch.Tensor, act1: bool, y: View, divisor: float = 1.0):
    """Conv(3->32, 3, 1) -> Conv(32->64, 3, 2) straight from the NCHW image into the NHWC view y (layer 0's output stays in LDS)."""
    require_gpu(x_nchw, "stem_pair")
    x = x_nchw.contiguous()
    n, c, h, w = x.shape
    check(_lib.lib().y3_stem_pair_fwd(x.data_ptr(), dtype_code(x.dtype), n, c, h, w, float(divisor), filt0.data_ptr(), bias0.data_ptr(), _lib.Y3_ACT_SILU if act0 else _lib.Y3_ACT_NONE,
                                      filt1.data_ptr(), bias1.data_ptr(), _lib.Y3_ACT_SILU if act1 else _lib.Y3_ACT_NONE, dtype_code(y.buf.dtype), _ref(y), stream_ptr()),
          "y3_stem_pair_fwd")


def pack_filter_pair(w_oihw: torch.Tensor, cout: int, cin: int, dtype: torch.dtype):
    """(forward bank, data-gradient bank) of one layer from its OIHW fp32 weights in one launch (training step)."""
    require_gpu(w_oihw, "pack_filter_pair")
    w = w_oihw.detach().to(torch.float32).contiguous()
    co, ci, k, _ = w.shape
    fwd = torch.empty(packed_filter_elems(cout, cin, k), dtype=dtype, device=w.device)
    dg = torch.empty(packed_filter_elems(cin, cout, k), dtype=dtype, device=w.device)
    check(_lib.lib().y3_pack_filter_pair(w.data_ptr(), co, ci, k, cout, cin, dtype_code(dtype), fwd.data_ptr(), dg.data_ptr(), stream_ptr()), "y3_pack_filter_pair")
    return fwd, dg


def shard_mean(parts: torch.Tensor, n_parts: int, n: int, scale: float, out: torch.Tensor):
    """out[i] = scale * (parts[0][i] + ... + parts[n_parts - 1][i]), fp32, summed in part order (parallel.GradBuckets: the owner's mean of its gradient shard)"""
    check(_lib.lib().y3_shard_mean(parts.data_ptr(), int(n_parts), int(n), float(scale), out.data_ptr(), stream_ptr()), "y3_shard_mean")


_anchor_ws: dict = {}


def _anchor_workspace(dev: torch.device, N: int, n: int, R: int) -> torch.Tensor:
    need = int(_lib.lib().y3_anchor_workspace_bytes(int(N), int(n), int(R)))
    if need == 0:
        check(-1, "y3_anchor_workspace_bytes")
    ws = _anchor_ws.get(dev.index)
    if ws is None or ws.numel() < need:
        ws = _anchor_ws[dev.index] = torch.empty(need, dtype=torch.uint8, device=dev)
    return ws


def _anchor_points(wh: torch.Tensor, what: str) -> torch.Tensor:
    require_gpu(wh, what)
    if wh.dtype != torch.float32 or wh.dim() != 2 or wh.shape[1] != 2 or not wh.is_contiguous():
        raise TypeError(f"{what} expects a contiguous (N, 2) fp32 table of label sizes")
    return wh


def anchor_metrics(wh: torch.Tensor, k: torch.Tensor, thr: float) -> torch.Tensor:
    """the six fp64 totals of y3_anchor_metrics for the (N, 2) fp32 sizes `wh` against the (n, 2) fp64 anchors `k`, both on the device; thr = 1 / anchor_t -> DEVICE (6,)"""
    wh = _anchor_points(wh, "anchor_metrics")
    require_gpu(k, "anchor_metrics")
    if k.dtype != torch.float64 or k.dim() != 2 or k.shape[1] != 2 or not k.is_contiguous():
        raise TypeError("anchor_metrics expects contiguous (n, 2) fp64 anchors")
    N, n = int(wh.shape[0]), int(k.shape[0])
    ws = _anchor_workspace(wh.device, max(N, 1), n, 0)
    totals = torch.empty(6, dtype=torch.float64, device=wh.device)
    check(_lib.lib().y3_anchor_metrics(wh.data_ptr(), N, k.data_ptr(), n, float(thr), totals.data_ptr(), ws.data_ptr(), ws.numel(), stream_ptr()), "y3_anchor_metrics")
    return totals


def anchor_evolve(wh: torch.Tensor, k: torch.Tensor, v: torch.Tensor, thr: float):
    """the genetic loop of kmean_anchors on the device (y3_anchor_evolve): k (n, 2) fp64 is evolved IN PLACE through the (gen, n, 2) fp64 mutations `v`
    -> (f (1,) fp64, accepted (gen,) int32), both on the device; nothing is read back"""
    wh = _anchor_points(wh, "anchor_evolve")
    require_gpu(k, "anchor_evolve")
    require_gpu(v, "anchor_evolve")
    if k.dtype != torch.float64 or v.dtype != torch.float64 or k.dim() != 2 or k.shape[1] != 2 or v.dim() != 3 or tuple(v.shape[1:]) != tuple(k.shape) or not k.is_contiguous() or not v.is_contiguous():
        raise TypeError("anchor_evolve expects contiguous fp64 anchors (n, 2) and mutations (gen, n, 2)")
    N, n, gen = int(wh.shape[0]), int(k.shape[0]), int(v.shape[0])
    ws = _anchor_workspace(wh.device, max(N, 1), n, 0)
    f = torch.zeros(1, dtype=torch.float64, device=wh.device)
    accepted = torch.zeros(max(gen, 1), dtype=torch.int32, device=wh.device)
    check(_lib.lib().y3_anchor_evolve(wh.data_ptr(), N, k.data_ptr(), f.data_ptr(), n, v.data_ptr() if gen else None, gen, float(thr), accepted.data_ptr(), ws.data_ptr(), ws.numel(),
                                      stream_ptr()), "y3_anchor_evolve")
    return f, accepted[:gen]


def kmeans_step(pts: torch.Tensor, codes: torch.Tensor, live: torch.Tensor, frozen: int, dist: torch.Tensor):
    """one Lloyd iteration of the R restarts that bit mask `frozen` leaves running (y3_kmeans_step): codes (R, n, 2) fp64 and live (R, n) int32 are updated in place,
    dist (R,) fp64 receives the mean distance under the old codes"""
    pts = _anchor_points(pts, "kmeans_step")
    for t in (codes, live, dist):
        require_gpu(t, "kmeans_step")
    R, n = int(codes.shape[0]), int(codes.shape[1])
    if codes.dtype != torch.float64 or dist.dtype != torch.float64 or live.dtype != torch.int32 or tuple(codes.shape) != (R, n, 2) or tuple(live.shape) != (R, n) or dist.numel() != R \
            or not (codes.is_contiguous() and live.is_contiguous() and dist.is_contiguous()):
        raise TypeError("kmeans_step expects contiguous codes (R, n, 2) fp64, live (R, n) int32 and dist (R,) fp64")
    N = int(pts.shape[0])
    ws = _anchor_workspace(pts.device, max(N, 1), n, R)
    check(_lib.lib().y3_kmeans_step(pts.data_ptr(), N, n, R, codes.data_ptr(), live.data_ptr(), int(frozen), dist.data_ptr(), ws.data_ptr(), ws.numel(), stream_ptr()), "y3_kmeans_step")


_choices_ws: dict = {}


def _label_classes(cls: torch.Tensor, what: str) -> torch.Tensor:
    require_gpu(cls, what)
    if cls.dtype != torch.float32 or cls.dim() != 1 or not cls.is_contiguous():
        raise TypeError(f"{what} expects the contiguous fp32 class column of the labels")
    return cls


def label_histogram(cls: torch.Tensor, nc: int) -> torch.Tensor:
    """the class histogram of the fp32 class column `cls` (N,) on the device (y3_label_histogram) -> DEVICE int32 (nc + 1,): labels per class, then the number of
    ids outside [0, nc)"""
    cls = _label_classes(cls, "label_histogram")
    N = int(cls.numel())
    counts = torch.empty(int(nc) + 1, dtype=torch.int32, device=cls.device)
    check(_lib.lib().y3_label_histogram(cls.data_ptr() if N else None, 1, N, counts.data_ptr(), int(nc), stream_ptr()), "y3_label_histogram")
    return counts


def image_weights(cls: torch.Tensor, offsets: torch.Tensor, class_weights: torch.Tensor) -> torch.Tensor:
    """iw[i] = sum of class_weights[id] over the labels [offsets[i], offsets[i + 1]) of image i (y3_image_weights): cls (N,) fp32, offsets (n + 1,) int64,
    class_weights (nc,) fp64, all on the device -> DEVICE fp64 (n,)"""
    cls = _label_classes(cls, "image_weights")
    require_gpu(offsets, "image_weights")
    require_gpu(class_weights, "image_weights")
    if offsets.dtype != torch.int64 or offsets.dim() != 1 or not offsets.is_contiguous() or class_weights.dtype != torch.float64 or class_weights.dim() != 1 \
            or not class_weights.is_contiguous():
        raise TypeError("image_weights expects contiguous int64 offsets (n + 1,) and fp64 class weights (nc,)")
    N, n = int(cls.numel()), int(offsets.numel()) - 1
    iw = torch.empty(max(n, 0), dtype=torch.float64, device=cls.device)
    check(_lib.lib().y3_image_weights(cls.data_ptr() if N else None, N, offsets.data_ptr(), n, class_weights.data_ptr(), int(class_weights.numel()), iw.data_ptr(), stream_ptr()),
          "y3_image_weights")
    return iw


def weighted_choices(weights: torch.Tensor, u: torch.Tensor) -> torch.Tensor:
    """random.choices(range(n), weights, k=len(u)) for the uniforms `u` on the device (y3_weighted_choices): weights (n,) and u (k,) fp64 -> DEVICE int64 (k + 1,):
    the k indices, then the status word (0, 1: total of weights not positive, 2: not finite)"""
    require_gpu(weights, "weighted_choices")
    require_gpu(u, "weighted_choices")
    if weights.dtype != torch.float64 or u.dtype != torch.float64 or weights.dim() != 1 or u.dim() != 1 or not weights.is_contiguous() or not u.is_contiguous():
        raise TypeError("weighted_choices expects contiguous fp64 weights (n,) and uniforms (k,)")
    n, k = int(weights.numel()), int(u.numel())
    need = int(_lib.lib().y3_weighted_choices_workspace_bytes(n))
    if need == 0:
        check(-1, "y3_weighted_choices_workspace_bytes")
    dev = weights.device
    ws = _choices_ws.get(dev.index)
    if ws is None or ws.numel() < need:
        ws = _choices_ws[dev.index] = torch.empty(need, dtype=torch.uint8, device=dev)
    out = torch.empty(k + 1, dtype=torch.int64, device=dev)
    check(_lib.lib().y3_weighted_choices(weights.data_ptr(), n, u.data_ptr() if k else None, k, out.data_ptr(), ws.data_ptr(), ws.numel(), stream_ptr()), "y3_weighted_choices")
    return out


def _dataset_args(what: str, images: torch.Tensor, n: int, indices: torch.Tensor | None, first: int, count: int):
    require_gpu(images, what)
    if images.dtype != torch.uint8 or images.dim() != 1 or not images.is_contiguous() or images.numel() != 32 * n:
        raise TypeError(f"{what} expects the contiguous record table of the set: uint8 ({32 * n},)")
    if indices is not None:
        require_gpu(indices, what)
        if indices.dtype != torch.int64 or indices.dim() != 1 or not indices.is_contiguous() or indices.numel() != count:
            raise TypeError(f"{what} expects {count} contiguous int64 indices")
    elif first < 0 or first + count > n:
        raise ValueError(f"{what}: images {first} .. {first + count - 1} lie outside the {n} of the set")


def dataset_batch(arena: torch.Tensor, images: torch.Tensor, n: int, indices: torch.Tensor | None, first: int, count: int, height: int, width: int,
                  dtype: torch.dtype = torch.uint8, out: torch.Tensor | None = None) -> torch.Tensor:
    """One batch of a device-resident dataset in one launch (y3_dataset_batch): `arena` the uint8 image arena, `images` its record table as bytes (32 n,), the batch
    the images indices[0 .. count) (DEVICE int64) or first .. first + count - 1 -> (count, 3, height, width) in `dtype` (uint8, or float16 / bfloat16 / float32
    divided by 255): letterboxed with 114, CHW, RGB.  `out`: a contiguous, 16-byte aligned tensor of that shape and dtype to write into."""
    what = "dataset_batch"
    require_gpu(arena, what)
    _dataset_args(what, images, n, indices, first, count)
    if arena.dtype != torch.uint8 or arena.dim() != 1 or not arena.is_contiguous():
        raise TypeError("dataset_batch expects the contiguous uint8 arena of the set")
    if dtype not in DTYPE_CODE:
        raise TypeError(f"dataset_batch writes uint8 / float16 / bfloat16 / float32, not {dtype}")
    shape = (int(count), 3, int(height), int(width))
    if out is None:
        out = torch.empty(shape, dtype=dtype, device=arena.device)
    elif tuple(out.shape) != shape or out.dtype != dtype or out.device != arena.device or not out.is_contiguous():
        raise TypeError(f"dataset_batch: `out` must be a contiguous {shape} {dtype} tensor on {arena.device}")
    if count:
        check(_lib.lib().y3_dataset_batch(arena.data_ptr(), arena.numel(), images.data_ptr(), int(n), _ptr(indices), int(first), int(count), out.data_ptr(), DTYPE_CODE[dtype],
                                          int(height), int(width), stream_ptr()), "y3_dataset_batch")
    return out


def dataset_targets(labels: torch.Tensor, label_offsets: torch.Tensor, images: torch.Tensor, n: int, indices: torch.Tensor | None, first: int, count: int, height: int,
                    width: int, n_rows: int):
    """The targets of one batch of a device-resident dataset (y3_dataset_targets): `labels` fp32 (total, 5) and `label_offsets` int64 (n + 1,) on the device, `n_rows`
    the batch's label count (the caller's host copy of the offsets knows it) -> (DEVICE fp32 (n_rows, 6) [image in batch, cls, x, y, w, h], DEVICE int64 (count + 1,)
    offsets): collate_fn's targets of the letterboxed images."""
    what = "dataset_targets"
    require_gpu(labels, what)
    require_gpu(label_offsets, what)
    _dataset_args(what, images, n, indices, first, count)
    if labels.dtype != torch.float32 or labels.dim() != 2 or labels.shape[1] != 5 or not labels.is_contiguous():
        raise TypeError("dataset_targets expects the contiguous fp32 (total, 5) label table")
    if label_offsets.dtype != torch.int64 or label_offsets.dim() != 1 or label_offsets.numel() != n + 1 or not label_offsets.is_contiguous():
        raise TypeError(f"dataset_targets expects {n + 1} contiguous int64 label offsets")
    targets = torch.empty(int(n_rows), 6, dtype=torch.float32, device=labels.device)
    offsets = torch.empty(int(count) + 1, dtype=torch.int64, device=labels.device)
    check(_lib.lib().y3_dataset_targets(labels.data_ptr() if labels.numel() else None, label_offsets.data_ptr(), images.data_ptr(), int(n), _ptr(indices), int(first), int(count),
                                        int(height), int(width), targets.data_ptr() if n_rows else None, int(n_rows), offsets.data_ptr(), stream_ptr()), "y3_dataset_targets")
    return targets, offsets


def dataset_stage_chunk_bytes() -> int:
    """the bytes one block of y3_dataset_stage copies: a job of the stage owns ceil(slot / this) chunks"""
    return int(_lib.lib().y3_dataset_stage_chunk_bytes())


def dataset_stage(host_arena: torch.Tensor, src_images: torch.Tensor, n: int, jobs: torch.Tensor, m: int, n_chunks: int, ring: torch.Tensor, dst_images: torch.Tensor,
                  status: torch.Tensor):
    """The images of one batch from a pinned HOST arena into a device ring, in one launch on the current stream (y3_dataset_stage): `host_arena` the uint8 arena in
    pinned host memory, `src_images` its record table on the device as bytes (32 n,), `jobs` DEVICE int64 (>= m, 3) [image, slot offset in `ring`, running chunk
    count], `n_chunks` the last count.  Writes the m slots of `ring` (DEVICE uint8; the image, then zeros up to the next multiple of 16) and the m records of
    `dst_images` (DEVICE uint8 (32 n,): the source record with the slot's offset); a job that does not fit is skipped and counted in `status` (DEVICE int32 (1,)).
    Whether `host_arena` is pinned, mapped host memory is the library's own check: it raises Y3Error and launches nothing for a pageable tensor."""
    what = "dataset_stage"
    for t in (src_images, jobs, ring, dst_images, status):
        require_gpu(t, what)
    if host_arena.is_cuda or host_arena.dtype != torch.uint8 or host_arena.dim() != 1 or not host_arena.is_contiguous():
        raise TypeError(f"{what} expects the contiguous uint8 arena of the set in host memory")
    for t in (src_images, dst_images):
        if t.dtype != torch.uint8 or t.dim() != 1 or not t.is_contiguous() or t.numel() != 32 * n:
            raise TypeError(f"{what} expects the contiguous record tables of the set: uint8 ({32 * n},)")
    if jobs.dtype != torch.int64 or jobs.dim() != 2 or jobs.shape[1] != 3 or not jobs.is_contiguous() or m < 0 or jobs.shape[0] < m:
        raise TypeError(f"{what} expects the contiguous int64 (m, 3) job table of the batch, m = {m}")
    if ring.dtype != torch.uint8 or ring.dim() != 1 or not ring.is_contiguous():
        raise TypeError(f"{what} expects a contiguous uint8 ring")
    if status.dtype != torch.int32 or status.numel() != 1:
        raise TypeError(f"{what} expects one int32 status word")
    _call("y3_dataset_stage", host_arena.data_ptr(), host_arena.numel(), src_images.data_ptr(), int(n), _data(jobs), int(m), int(n_chunks), ring.data_ptr(), ring.numel(),
          dst_images.data_ptr(), status.data_ptr())


AUGMENT_ITEM_BYTES = 1360   # sizeof(y3_augment_item)


# The augment wrappers.  Every argument group has one validator, whose refusal carries `what`, the name of the public wrapper the caller used; a public wrapper is its
# refusals in their order, the allocation of what its export writes, and _call.  `batch`: what _augment_args returns, (images, n, items, count) as the exports take them.


def _augment_args(what: str, images: torch.Tensor, n: int, items: torch.Tensor, count: int, *sides: int):
    require_gpu(images, what)
    require_gpu(items, what)
    if images.dtype != torch.uint8 or images.dim() != 1 or not images.is_contiguous() or images.numel() != 32 * n:
        raise TypeError(f"{what} expects the contiguous record table of the set: uint8 ({32 * n},)")
    if items.dtype != torch.uint8 or items.dim() != 1 or not items.is_contiguous() or count < 0 or items.numel() < AUGMENT_ITEM_BYTES * count:
        raise TypeError(f"{what} expects the contiguous item records of the batch: uint8, at least {AUGMENT_ITEM_BYTES * count} bytes")
    for size in sides:
        if size < 16 or size % 16:
            raise ValueError(f"{what}: the image size {size} is not a multiple of 16")
    return images.data_ptr(), int(n), items.data_ptr(), int(count)


def _table(what: str, t: torch.Tensor, cols: int, name: str, nonempty: bool = False):
    """the label table (cols 5, name "(total, 5) label") or the vertex table (2, "(V, 2) vertex") of the set"""
    if t.dtype != torch.float32 or t.dim() != 2 or t.shape[1] != cols or not t.is_contiguous() or (nonempty and not t.numel()):
        raise TypeError(f"{what} expects the contiguous{', non-empty' if nonempty else ''} fp32 {name} table")


def _offsets(what: str, t: torch.Tensor, k: int | None, name: str):
    """the int64 offsets of the label table (k = images + 1) or of the vertex table (k = label rows + 1; None: one at least)"""
    if t.dtype != torch.int64 or t.dim() != 1 or not t.is_contiguous() or (t.numel() < 1 if k is None else t.numel() != k):
        raise TypeError(f"{what} expects contiguous int64 {name} offsets, one per label row plus one" if k is None else f"{what} expects {k} contiguous int64 {name} offsets")


def _arena(what: str, arena: torch.Tensor, dtype: torch.dtype):
    if arena.dtype != torch.uint8 or arena.dim() != 1 or not arena.is_contiguous():
        raise TypeError(f"{what} expects the contiguous uint8 arena of the set")
    if dtype not in DTYPE_CODE:
        raise TypeError(f"{what} writes uint8 / float16 / bfloat16 / float32, not {dtype}")


def _out(what: str, out: torch.Tensor | None, shape: tuple, dtype: torch.dtype, device) -> torch.Tensor:
    if out is None:
        return torch.empty(shape, dtype=dtype, device=device)
    if tuple(out.shape) != shape or out.dtype != dtype or out.device != device or not out.is_contiguous():
        raise TypeError(f"{what}: `out` must be a contiguous {shape} {dtype} tensor on {device}")
    return out


def _polygon_workspace(what: str, n_rows: int, count: int, device=None, given=None):
    """(boxes, inside, paths) of a batch: allocated on `device`, or `given` checked to be what augment_polygons allocated for it"""
    spec = ((torch.float64, (int(n_rows), 4)), (torch.int32, (int(n_rows),)), (torch.int32, (int(count), 2)))
    if given is None:
        return tuple(torch.empty(shape, dtype=dt, device=device) for dt, shape in spec)
    for t, (dt, shape) in zip(given, spec):
        require_gpu(t, what)
        if t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous():
            raise TypeError(f"{what} expects the contiguous {dt} {shape} workspace of augment_polygons")
    return given


def _data(t: torch.Tensor):
    return t.data_ptr() if t.numel() else None


def _call(export: str, *args):
    check(getattr(_lib.lib(), export)(*args, stream_ptr()), export)


def _polygons(export: str, vertices, vertex_offsets, label_offsets, batch, size, n_rows, paste=()):
    ws = _polygon_workspace(export, n_rows, batch[3], vertices.device)
    _call(export, _data(vertices), vertices.shape[0], vertex_offsets.data_ptr(), vertex_offsets.numel() - 1, label_offsets.data_ptr(), *batch, int(size), *paste,
          *map(_data, ws), int(n_rows))
    return ws


def _targets(export: str, labels, label_offsets, batch, sides, n_rows, ws=(), paste=()):
    targets = torch.empty(int(n_rows), 6, dtype=torch.float32, device=labels.device)
    offsets = torch.empty(batch[3] + 1, dtype=torch.int64, device=labels.device)
    _call(export, _data(labels), label_offsets.data_ptr(), *batch, *map(int, sides), *paste, *map(_data, ws), _data(targets), int(n_rows), offsets.data_ptr())
    return targets, offsets


def _augment_batch(what: str, export: str, arena, images, n, items, count, sides, dtype, out):
    """augment_batch (sides = (S,)) and augment_batch_hw (sides = (H, W)), each with its own export"""
    require_gpu(arena, what)
    batch = _augment_args(what, images, n, items, count, *sides)
    _arena(what, arena, dtype)
    out = _out(what, out, (int(count), 3, int(sides[0]), int(sides[-1])), dtype, arena.device)
    if count:
        _call(export, arena.data_ptr(), arena.numel(), *batch, out.data_ptr(), DTYPE_CODE[dtype], *map(int, sides))
    return out


def augment_batch(arena: torch.Tensor, images: torch.Tensor, n: int, items: torch.Tensor, count: int, size: int, dtype: torch.dtype = torch.uint8,
                  out: torch.Tensor | None = None) -> torch.Tensor:
    """One augmented batch of a device-resident dataset in one launch (y3_augment_batch): `arena` / `images` as for dataset_batch, `items` the batch's
    y3_augment_item records as bytes (1360 each, what augment.pack_items forms) -> (count, 3, size, size) in `dtype`: mosaic, affine warp, mixup, HSV and the flips
    applied, CHW, RGB.  `out`: a contiguous, 16-byte aligned tensor of that shape and dtype to write into."""
    return _augment_batch("augment_batch", "y3_augment_batch", arena, images, n, items, count, (size,), dtype, out)


def augment_batch_hw(arena: torch.Tensor, images: torch.Tensor, n: int, items: torch.Tensor, count: int, height: int, width: int, dtype: torch.dtype = torch.uint8,
                     out: torch.Tensor | None = None) -> torch.Tensor:
    """augment_batch for items of `height` rows and `width` columns, the batch shape of a rect=True set (y3_augment_batch_hw; both multiples of 16) ->
    (count, 3, height, width) in `dtype`."""
    return _augment_batch("augment_batch_hw", "y3_augment_batch_hw", arena, images, n, items, count, (height, width), dtype, out)


def _augment_targets(what: str, export: str, labels, label_offsets, images, n, items, count, sides, n_rows, ws=()):
    """the targets wrappers without a paste, each with its own export: sides = (S,) or (H, W), `ws` the workspace of the polygon form"""
    require_gpu(labels, what)
    require_gpu(label_offsets, what)
    batch = _augment_args(what, images, n, items, count, *sides)
    _table(what, labels, 5, "(total, 5) label")
    _offsets(what, label_offsets, n + 1, "label")
    return _targets(export, labels, label_offsets, batch, sides, n_rows, ws and _polygon_workspace(what, n_rows, count, given=ws))


def augment_targets(labels: torch.Tensor, label_offsets: torch.Tensor, images: torch.Tensor, n: int, items: torch.Tensor, count: int, size: int, n_rows: int):
    """The targets of one augmented batch (y3_augment_targets): `n_rows` the label count of all tiles of the batch, an upper bound of the survivors ->
    (DEVICE fp32 (n_rows, 6) [item in batch, cls, x, y, w, h], DEVICE int64 (count + 1,) offsets); only the first offsets[count] rows are written."""
    return _augment_targets("augment_targets", "y3_augment_targets", labels, label_offsets, images, n, items, count, (size,), n_rows)


def augment_targets_hw(labels: torch.Tensor, label_offsets: torch.Tensor, images: torch.Tensor, n: int, items: torch.Tensor, count: int, height: int, width: int, n_rows: int):
    """augment_targets for items of `height` rows and `width` columns (y3_augment_targets_hw): the boxes are clipped and normalised per axis."""
    return _augment_targets("augment_targets_hw", "y3_augment_targets_hw", labels, label_offsets, images, n, items, count, (height, width), n_rows)


def augment_polygons(vertices: torch.Tensor, vertex_offsets: torch.Tensor, label_offsets: torch.Tensor, images: torch.Tensor, n: int, items: torch.Tensor, count: int,
                     size: int, n_rows: int):
    """The polygon boxes of one augmented batch (y3_augment_polygons), the launch ahead of augment_targets_polygons: `vertices` fp32 (V, 2) and `vertex_offsets` int64
    (label rows + 1,) of the set on the device, `n_rows` as for augment_targets -> (DEVICE fp64 (n_rows, 4) segment2box of every label position of the batch's mosaics,
    DEVICE int32 (n_rows,) whether a point lay inside, DEVICE int32 (count, 2) the path word per item and mosaic: 1 = the polygon path).  Positions of letterbox items
    are not written."""
    what = "augment_polygons"
    for t in (vertices, vertex_offsets, label_offsets):
        require_gpu(t, what)
    batch = _augment_args(what, images, n, items, count, size)
    _table(what, vertices, 2, "(V, 2) vertex")
    _offsets(what, vertex_offsets, None, "vertex")
    _offsets(what, label_offsets, n + 1, "label")
    return _polygons("y3_augment_polygons", vertices, vertex_offsets, label_offsets, batch, size, n_rows)


def augment_targets_polygons(labels: torch.Tensor, label_offsets: torch.Tensor, images: torch.Tensor, n: int, items: torch.Tensor, count: int, size: int, n_rows: int,
                             boxes: torch.Tensor, inside: torch.Tensor, paths: torch.Tensor):
    """augment_targets for a set with polygon labels (y3_augment_targets_polygons): `boxes`, `inside`, `paths` as augment_polygons returned them for this batch; a mosaic
    whose path word is 1 takes the polygon boxes with area_thr 0.01, every other the four corners with 0.10."""
    return _augment_targets("augment_targets_polygons", "y3_augment_targets_polygons", labels, label_offsets, images, n, items, count, (size,), n_rows, (boxes, inside, paths))


_paste_ws: dict = {}   # device -> the int32 words of the copy-paste masks, grown on demand and cleared per batch


def augment_copy_paste(labels: torch.Tensor, label_offsets: torch.Tensor, vertices: torch.Tensor, vertex_offsets: torch.Tensor, arena: torch.Tensor, images: torch.Tensor,
                       n: int, items: torch.Tensor, count: int, size: int, n_rows: int, paste: torch.Tensor, n_paste: int, n_masks: int,
                       dtype: torch.dtype = torch.uint8, out: torch.Tensor | None = None):
    """One augmented batch of a set with polygon labels in which some mosaic pastes (copy_paste inside load_mosaic): the five launches y3_augment_copy_paste_select,
    y3_augment_copy_paste_raster, y3_augment_batch_paste, y3_augment_polygons_paste and y3_augment_targets_paste on the caller's stream.  `paste`: the DEVICE int32
    table of the batch (augment.pack_paste: 2 count + 1 offsets, 2 count mask indices, the n_paste candidates), `n_masks` the mosaics with candidates, `n_rows` the
    label count of all tiles plus n_paste.  The masks are a workspace of this module, (n_masks, 2 size, 2 size / 32) int32 words, cleared here: the view returned is
    good until the next call on the same device.
    -> (im, targets, offsets, (boxes, inside, paths), (sel_i (n_paste, 4) int32 [accepted, j, polygon row, tile], sel_f (n_paste, 5) fp32 [cls, box], masks))"""
    what = "augment_copy_paste"
    for t in (labels, label_offsets, vertices, vertex_offsets, arena, paste):
        require_gpu(t, what)
    batch = _augment_args(what, images, n, items, count, size)
    _table(what, labels, 5, "(total, 5) label", nonempty=True)
    _table(what, vertices, 2, "(V, 2) vertex", nonempty=True)
    _offsets(what, label_offsets, n + 1, "label")
    _offsets(what, vertex_offsets, labels.shape[0] + 1, "vertex")
    _arena(what, arena, dtype)
    n_paste, n_masks, count, size, n_rows = int(n_paste), int(n_masks), int(count), int(size), int(n_rows)
    if count < 1 or n_paste < 1 or not 1 <= n_masks <= 2 * count or n_rows < n_paste:
        raise ValueError(f"{what}: {n_paste} candidates in {n_masks} mosaics of {count} items, {n_rows} rows")
    if paste.dtype != torch.int32 or paste.dim() != 1 or not paste.is_contiguous() or paste.numel() != 4 * count + 1 + n_paste:
        raise TypeError(f"{what} expects the contiguous int32 paste table of the batch: {4 * count + 1 + n_paste} words")
    dev = labels.device
    out = _out(what, out, (count, 3, size, size), dtype, dev)
    words = n_masks * 2 * size * (2 * size // 32)
    ws = _paste_ws.get(dev)
    if ws is None or ws.numel() < words:
        ws = _paste_ws[dev] = torch.empty(words, dtype=torch.int32, device=dev)
    masks = ws[:words].zero_()
    sel_i = torch.empty(n_paste, 4, dtype=torch.int32, device=dev)
    sel_f = torch.empty(n_paste, 5, dtype=torch.float32, device=dev)
    n_vertices, n_label_rows = vertices.shape[0], vertex_offsets.numel() - 1
    selection = (paste.data_ptr(), n_paste, sel_i.data_ptr(), sel_f.data_ptr())   # (paste, n_paste, sel_i, sel_f) as the three exports after the raster take them
    _call("y3_augment_copy_paste_select", labels.data_ptr(), label_offsets.data_ptr(), vertex_offsets.data_ptr(), n_vertices, n_label_rows, *batch, size, *selection)
    _call("y3_augment_copy_paste_raster", vertices.data_ptr(), n_vertices, vertex_offsets.data_ptr(), n_label_rows, label_offsets.data_ptr(), *batch, size,
          paste.data_ptr(), n_paste, sel_i.data_ptr(), masks.data_ptr(), n_masks)
    _call("y3_augment_batch_paste", arena.data_ptr(), arena.numel(), *batch, out.data_ptr(), DTYPE_CODE[dtype], size, paste.data_ptr(), masks.data_ptr(), n_masks)
    polygons = _polygons("y3_augment_polygons_paste", vertices, vertex_offsets, label_offsets, batch, size, n_rows, selection)
    targets, offsets = _targets("y3_augment_targets_paste", labels, label_offsets, batch, (size,), n_rows, polygons, selection)
    return out, targets, offsets, polygons, (sel_i, sel_f, masks.view(n_masks, 2 * size, 2 * size // 32))


# The classifier-crop wrappers (csrc/crops.hip), organised as the augment wrappers above: one validator per argument group, each refusal carrying `what`.
CROP_DTYPES = (torch.float16, torch.bfloat16, torch.float32)
CROP_MAX_SIZE = 1024


def _detections(what: str, rows: torch.Tensor, counts: torch.Tensor):
    """the padded NMS result: rows fp32 (bs, max_rows, >= 6) with unit stride along a row, counts DEVICE int32 (bs,) -> (rows, img_stride, row_stride, counts, bs, max_rows)
    as the exports take them"""
    require_gpu(rows, what)
    require_gpu(counts, what)
    if rows.dtype != torch.float32 or rows.dim() != 3 or rows.shape[2] < 6 or (rows.numel() and rows.stride(2) != 1):
        raise TypeError(f"{what} expects the fp32 (bs, max_det, 6) rows of non_max_suppression_batched")
    if counts.dtype != torch.int32 or counts.dim() != 1 or counts.numel() != rows.shape[0] or not counts.is_contiguous():
        raise TypeError(f"{what} expects {rows.shape[0]} contiguous int32 counts, one per image")
    return rows.data_ptr(), int(rows.stride(0)), int(rows.stride(1)), counts.data_ptr(), int(rows.shape[0]), int(rows.shape[1])


def _box_table(what: str, boxes: torch.Tensor, bs: int, max_rows: int):
    require_gpu(boxes, what)
    if boxes.dtype != torch.float32 or tuple(boxes.shape) != (bs, max_rows, 4) or not boxes.is_contiguous():
        raise TypeError(f"{what} expects the contiguous fp32 ({bs}, {max_rows}, 4) box table of classifier_boxes")


def _tiles(what: str, prefix: torch.Tensor, bs: int, max_rows: int, n_tiles: int):
    require_gpu(prefix, what)
    if prefix.dtype != torch.int64 or prefix.dim() != 1 or prefix.numel() != bs or not prefix.is_contiguous():
        raise TypeError(f"{what} expects {bs} contiguous int64 prefix entries, one per image")
    if not 0 <= n_tiles <= bs * max_rows:
        raise ValueError(f"{what}: {n_tiles} crops of {bs} images with at most {max_rows} detections each")


def _image_set(what: str, arena: torch.Tensor, images: torch.Tensor, bs: int):
    """the arena and the record table of the batch's source images (crops.DeviceImages): one record per image of the batch"""
    require_gpu(arena, what)
    require_gpu(images, what)
    if arena.dtype != torch.uint8 or arena.dim() != 1 or not arena.is_contiguous() or arena.numel() < 4 or arena.numel() % 4:
        raise TypeError(f"{what} expects the contiguous uint8 arena of the images, a positive multiple of 4 bytes")
    if images.dtype != torch.uint8 or images.dim() != 1 or not images.is_contiguous() or images.numel() % 32:
        raise TypeError(f"{what} expects the contiguous record table of the images: uint8, 32 bytes each")
    if images.numel() != 32 * bs:
        raise ValueError(f"{what}: {images.numel() // 32} images for the detections of {bs}")
    return images.data_ptr(), int(bs)


def classifier_boxes(rows: torch.Tensor, counts: torch.Tensor, gain: float = 1.3, pad: float = 30.0, square: bool = True) -> torch.Tensor:
    """The padded, squared, truncated boxes of apply_classifier in one launch (y3_classifier_boxes): `rows` / `counts` the DEVICE output of non_max_suppression_batched
    in the letterboxed space -> DEVICE fp32 (bs, max_det, 4), zeros at and beyond an image's count.  `rows` is not written.  square=False, gain=1.02, pad=10: the box
    of upstream save_one_box."""
    what = "classifier_boxes"
    det = _detections(what, rows, counts)
    boxes = torch.empty(det[4], det[5], 4, dtype=torch.float32, device=rows.device)
    if boxes.numel():
        _call("y3_classifier_boxes", *det, float(gain), float(pad), 1 if square else 0, boxes.data_ptr())
    return boxes


def crop_resize(arena: torch.Tensor, images: torch.Tensor, boxes: torch.Tensor, counts: torch.Tensor, prefix: torch.Tensor, n_tiles: int, size: int = 224,
                dtype: torch.dtype = torch.float32, status: torch.Tensor | None = None, out: torch.Tensor | None = None):
    """The crops of a batch in one launch (y3_crop_resize): `arena` / `images` the source images and their records (32 bs,), `boxes` the scaled, clipped table of
    classifier_boxes + scale_boxes, `prefix` DEVICE int64 (bs,) the exclusive prefix of `counts`, `n_tiles` their sum as the host knows it ->
    (DEVICE (n_tiles, 3, size, size) in `dtype`: RGB, CHW, divided by 255; status DEVICE int32 (1,): the crops written as zeros)."""
    what = "crop_resize"
    bs, max_rows = int(boxes.shape[0]), int(boxes.shape[1]) if boxes.dim() == 3 else 0
    _box_table(what, boxes, bs, max_rows)
    require_gpu(counts, what)
    if counts.dtype != torch.int32 or counts.dim() != 1 or counts.numel() != bs or not counts.is_contiguous():
        raise TypeError(f"{what} expects {bs} contiguous int32 counts, one per image")
    n_tiles, size = int(n_tiles), int(size)
    _tiles(what, prefix, bs, max_rows, n_tiles)
    if not 1 <= size <= CROP_MAX_SIZE:
        raise ValueError(f"{what}: size = {size}; crops are 1 .. {CROP_MAX_SIZE} pixels on a side")
    if dtype not in CROP_DTYPES:
        raise TypeError(f"{what} writes float16 / bfloat16 / float32, not {dtype}")
    if status is None:
        status = torch.zeros(1, dtype=torch.int32, device=boxes.device)
    elif not status.is_cuda or status.dtype != torch.int32 or status.numel() != 1:
        raise TypeError(f"{what} expects one int32 status word on the device")
    out = _out(what, out, (n_tiles, 3, size, size), dtype, boxes.device)
    if n_tiles:
        batch = _image_set(what, arena, images, bs)
        _call("y3_crop_resize", arena.data_ptr(), arena.numel(), *batch, boxes.data_ptr(), counts.data_ptr(), prefix.data_ptr(), bs, max_rows, out.data_ptr(), DTYPE_CODE[dtype],
              n_tiles, size, status.data_ptr())
    return out, status


def keep_matching(rows: torch.Tensor, counts: torch.Tensor, prefix: torch.Tensor, classes: torch.Tensor, boxes: torch.Tensor, arena: torch.Tensor, images: torch.Tensor):
    """The filter of apply_classifier in one launch (y3_keep_matching): `classes` DEVICE int64 (n_tiles,), the classifier's class per crop ->
    (DEVICE fp32 (bs, max_det, 6): per image the rows whose (long) cls equals the class of their crop, in order, then zeros; DEVICE int32 (bs,) the new counts).
    A crop the status word of crop_resize counted never matches."""
    what = "keep_matching"
    det = _detections(what, rows, counts)
    bs, max_rows = det[4], det[5]
    _box_table(what, boxes, bs, max_rows)
    require_gpu(classes, what)
    if classes.dtype != torch.int64 or classes.dim() != 1 or not classes.is_contiguous():
        raise TypeError(f"{what} expects the contiguous int64 classes of the crops")
    _tiles(what, prefix, bs, max_rows, int(classes.numel()))
    out = torch.empty(bs, max_rows, 6, dtype=torch.float32, device=rows.device)
    out_counts = torch.empty(bs, dtype=torch.int32, device=rows.device)
    if bs and max_rows:
        batch = _image_set(what, arena, images, bs)
        _call("y3_keep_matching", *det[:4], prefix.data_ptr(), bs, max_rows, _data(classes), int(classes.numel()), boxes.data_ptr(), *batch, arena.numel(), out.data_ptr(),
              out_counts.data_ptr())
    else:
        out_counts.zero_()
    return out, out_counts


_coco_ws: dict = {}


def _coco_check(what: str, **tensors):
    """every tensor on the device, contiguous, of the dtype its name's suffix says (name__dtype)"""
    for name, t in tensors.items():
        label, dt = name.rsplit("__", 1)
        require_gpu(t, what)
        if t.dtype != getattr(torch, dt) or not t.is_contiguous():
            raise TypeError(f"{what} expects contiguous {dt} {label}")


def coco_match(det_img, det_cat, det_box, det_score, img_ids, cat_ids, gt_box, gt_area, gt_crowd, gt_cat, gt_offsets, iou_thrs, area_rng, max_det: int):
    """COCOeval.computeIoU + evaluateImg for every (image, category) pair on the device (y3_coco_match; include/yolov3_hip.h has the layouts) -> dict of DEVICE tensors:
    score fp64 (N,), rank int32 (N,), match / ignore uint16 (N, A) -- the rows in accumulate order -- cat_begin / cat_end int32 (K,), npig int32 (K, A)"""
    what = "coco_match"
    _coco_check(what, det_img__int64=det_img, det_cat__int64=det_cat, det_box__float64=det_box, det_score__float64=det_score, img_ids__int64=img_ids, cat_ids__int64=cat_ids,
                gt_box__float64=gt_box, gt_area__float64=gt_area, gt_crowd__uint8=gt_crowd, gt_cat__int32=gt_cat, gt_offsets__int32=gt_offsets, iou_thrs__float64=iou_thrs,
                area_rng__float64=area_rng)
    N, G, n_img, K, T, A = int(det_score.numel()), int(gt_area.numel()), int(img_ids.numel()), int(cat_ids.numel()), int(iou_thrs.numel()), int(area_rng.numel()) // 2
    if det_img.numel() != N or det_cat.numel() != N or det_box.numel() != 4 * N or gt_box.numel() != 4 * G or gt_crowd.numel() != G or gt_cat.numel() != G \
            or gt_offsets.numel() != n_img * K + 1 or area_rng.numel() != 2 * A:
        raise ValueError("coco_match: the detection / ground-truth columns and the offsets do not have the sizes of one table")
    dev = det_score.device
    need = int(_lib.lib().y3_coco_eval_workspace_bytes(N, G, T, A))
    if need == 0:
        check(-1, "y3_coco_eval_workspace_bytes")
    ws = _coco_ws.get(dev.index)
    if ws is None or ws.numel() < need:
        ws = _coco_ws[dev.index] = torch.empty(need, dtype=torch.uint8, device=dev)
    out = dict(score=torch.empty(N, dtype=torch.float64, device=dev), rank=torch.empty(N, dtype=torch.int32, device=dev),
               match=torch.empty(N, A, dtype=torch.uint16, device=dev), ignore=torch.empty(N, A, dtype=torch.uint16, device=dev),
               cat_begin=torch.empty(K, dtype=torch.int32, device=dev), cat_end=torch.empty(K, dtype=torch.int32, device=dev), npig=torch.empty(K, A, dtype=torch.int32, device=dev))
    p = lambda t: t.data_ptr() if t.numel() else None   # noqa: E731
    check(_lib.lib().y3_coco_match(p(det_img), p(det_cat), p(det_box), p(det_score), N, img_ids.data_ptr(), n_img, cat_ids.data_ptr(), K, p(gt_box), p(gt_area), p(gt_crowd), p(gt_cat),
                                   G, gt_offsets.data_ptr(), iou_thrs.data_ptr(), T, area_rng.data_ptr(), A, int(max_det), p(out["score"]), p(out["rank"]), p(out["match"]),
                                   p(out["ignore"]), out["cat_begin"].data_ptr(), out["cat_end"].data_ptr(), out["npig"].data_ptr(), ws.data_ptr(), ws.numel(), stream_ptr()),
          "y3_coco_match")
    return out


def coco_accumulate(rows: dict, T: int, rec_thrs: torch.Tensor, max_dets: torch.Tensor):
    """COCOeval.accumulate over the rows `coco_match` returned (y3_coco_accumulate) -> DEVICE fp64 precision (T, R, K, A, M), recall (T, K, A, M), scores (T, R, K, A, M)"""
    what = "coco_accumulate"
    _coco_check(what, score__float64=rows["score"], rank__int32=rows["rank"], match__uint16=rows["match"], ignore__uint16=rows["ignore"], cat_begin__int32=rows["cat_begin"],
                cat_end__int32=rows["cat_end"], npig__int32=rows["npig"], rec_thrs__float64=rec_thrs, max_dets__int32=max_dets)
    N, (K, A), R, M = int(rows["score"].numel()), rows["npig"].shape, int(rec_thrs.numel()), int(max_dets.numel())
    dev = rec_thrs.device
    precision = torch.empty(T, R, K, A, M, dtype=torch.float64, device=dev)
    scores = torch.empty(T, R, K, A, M, dtype=torch.float64, device=dev)
    recall = torch.empty(T, K, A, M, dtype=torch.float64, device=dev)
    p = lambda t: t.data_ptr() if t.numel() else None   # noqa: E731
    check(_lib.lib().y3_coco_accumulate(p(rows["score"]), p(rows["rank"]), p(rows["match"]), p(rows["ignore"]), N, rows["cat_begin"].data_ptr(), rows["cat_end"].data_ptr(),
                                        rows["npig"].data_ptr(), int(K), int(T), rec_thrs.data_ptr(), R, max_dets.data_ptr(), M, int(A), precision.data_ptr(), scores.data_ptr(),
                                        recall.data_ptr(), stream_ptr()), "y3_coco_accumulate")
    return precision, recall, scores
