"""-m gpu: every conv and training kernel on channel-sliced views.

The engines never copy for Concat: a layer that feeds one is placed inside the concat buffer, so its consumers read an input, a shortcut or a gradient whose pitch exceeds its
channel count and whose data pointer is offset (ops.View / y3_tensor: "channels [coff, coff + c) of a (n, h, w, pitch) buffer and nothing else").  Per kernel and sliced case:
  1. the fp32 / fp64 CPU reference of the contiguous test of that kernel, with that test's tolerance (no new tolerances; the few derived bounds are derived where they stand);
  2. bit identity with the same problem on pitch == c tensors -- pitch changes addresses, not tiling or accumulation order -- and the same variant / plan for both;
  3. poison and canary: NaN everywhere outside the input slices, a canary outside the output slice; the output must be finite, canary and inputs bit-unchanged.
A kernel that rounds K up and leans on zero filter padding multiplies the neighbour's channels by zero: 0 * NaN shows up in (3).
"""
import math

import pytest
import torch
import torch.nn.functional as F

from test_gpu_parity import (BNECK_CASES, BNIN_CASES, CONV_CASES, KSPLIT_CASES, S1X1_CASES, STRIP_CONV_CASES, V10_CASES, _bn_reference, _conv_tol_check, _ops,
                             assert_outside_unchanged, bits, conv_ws, run_conv, wide_view)

pytestmark = pytest.mark.gpu

NAN = float("nan")
HALVES = [torch.float16, torch.bfloat16]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


def _case(table, name):
    return next(c for c in table if c[0] == name)


class Buf:
    """a tensor of a launch: `c` channels inside a wider buffer (pads = (left, right) channels, None = pitch == c), the rest poison (inputs: NaN) or canary (outputs)"""

    def __init__(self, ops, dev, dtype, shape, pads, fill=NAN, data=None):
        n, h, w, c = shape
        self.big, self.v = wide_view(ops, n, h, w, c, dtype, dev, pads, fill)
        if data is not None:
            self.v.as_nhwc().copy_(data.to(dev).to(dtype))
        self.before = None

    def snap(self):
        self.before = self.big.buf.clone()
        return self

    def check(self, what, written=False):
        assert_outside_unchanged(self.big, self.before, [(self.v.coff, self.v.c)] if written else [], what)

    def nhwc(self):
        return self.v.as_nhwc().clone()


# pads (left, right) in channels; different on the two sides and from tensor to tensor, pitches stay multiples of 8, slice starts 16-byte aligned (8 halves / 4 floats)
PX, PR, PY = (16, 24), (32, 8), (8, 40)
X_ONLY = {"x": PX}
RES_ONLY = {"res": PR}
ALL3 = {"x": PX, "res": PR, "y": PY}
XY = {"x": PX, "y": PY}
SAME_BUF = {"x": PX, "res": (16, 0), "y": (24, 8), "res_in_y": True}   # [16 | shortcut | 24 | output | 8]: the last Bottleneck of a C3-style stage inside its concat buffer

V10_KNOBS = {"conv_v10": 2}
KSPLIT_KNOBS = {"conv_v10": 2, "v10_ksplit": 2}

FWD_SLICED = [
    # id, (n,h,w,cin,cout,k,s), run_conv kwargs, knobs, workspace, expected variant, views
    ("v3_bk32_x_y", _case(CONV_CASES, "3x3s1_bk64_tc128")[1], {}, {}, False, "v3_bk32_128x128", XY),
    ("v3_bk32_res_x_only", _case(CONV_CASES, "residual")[1], {"residual": True}, {}, False, "v3_bk32_128x128", X_ONLY),
    ("v3_bk32_res_res_only", _case(CONV_CASES, "residual")[1], {"residual": True}, {}, False, "v3_bk32_128x128", RES_ONLY),
    ("v3_bk32_res_all", _case(CONV_CASES, "residual")[1], {"residual": True}, {}, False, "v3_bk32_128x128", ALL3),
    ("v3_bk32_res_same_buffer", _case(CONV_CASES, "residual")[1], {"residual": True}, {}, False, "v3_bk32_128x128", SAME_BUF),
    ("v3_bk32_partial_tiles", _case(CONV_CASES, "partial_tiles")[1], {"residual": True}, {}, False, "v3_bk32_128x128", ALL3),
    ("v3_bk64_s2", _case(CONV_CASES, "3x3s2_bk64_tc128")[1], {"residual": True}, {}, False, "v3_bk64_128x128", ALL3),
    ("v3_bk64_1x1_k768", _case(CONV_CASES, "1x1_k768_concat_in")[1], {}, {}, False, "v3_bk64_128x128", XY),
    ("v3_bk64_head_255", _case(CONV_CASES, "head_255")[1], {"cout_real": 255, "act": False}, {}, False, "v3_bk64_128x128", XY),
    ("v3_64x256_cout64", _case(CONV_CASES, "3x3s1_bk32_tc64")[1], {"residual": True}, {}, False, "v3_bk32_64x256", ALL3),
    ("v3_64x256_1x1_cout32", _case(CONV_CASES, "1x1_cout32")[1], {}, {}, False, "v3_bk32_64x256", XY),
    ("v6_big_k", _case(CONV_CASES, "big_k_3x3_512")[1], {"residual": True}, {}, False, "v6", ALL3),
    ("v6_same_buffer", _case(CONV_CASES, "big_k_3x3_512")[1], {"residual": True}, {}, False, "v6", SAME_BUF),
    ("v2_smallc_cin3", _case(CONV_CASES, "first_layer_cin3")[1], {"cin_real": 3, "residual": True}, {}, False, "v2_smallc", ALL3),      # Cin = 8: K = 72 rounds up to 96
    ("v2_smallc_cin16", _case(CONV_CASES, "tiny_cin16")[1], {"residual": True}, {}, False, "v2_smallc", ALL3),                           # Cin = 16: K = 144 rounds up to 160
    ("v2_smallc_cin16_x_only", _case(CONV_CASES, "tiny_cin16")[1], {}, {}, False, "v2_smallc", X_ONLY),
    ("upsample_scatter", _case(CONV_CASES, "upsample_scatter")[1], {"ups": True}, {}, False, "v3_bk64_128x128", XY),
    ("v10_res_all", _case(V10_CASES, "plan_20x20_res")[1], {"residual": True}, {**V10_KNOBS, "v10_half": 0}, True, "v10", ALL3),
    ("v10_res_same_buffer", _case(V10_CASES, "plan_20x20_res")[1], {"residual": True}, {**V10_KNOBS, "v10_half": 0}, True, "v10", SAME_BUF),
    ("v10_odd_cb_x_only", _case(V10_CASES, "odd_cb_parity")[1], {}, {**V10_KNOBS, "v10_half": 0, "v10_mp": 6, "v10_blocks": 2}, True, "v10", X_ONLY),
    ("v10h_res_all", _case(V10_CASES, "plan_20x20_res")[1], {"residual": True}, {**V10_KNOBS, "v10_half": 1}, True, "v10h", ALL3),
    ("v10h_tiny_images_res_only", _case(V10_CASES, "tiny_images_one_cb")[1], {"residual": True}, {**V10_KNOBS, "v10_half": 1, "v10_mp": 4, "v10_blocks": 3}, True, "v10h", RES_ONLY),
    ("v10k_res_3_slices", _case(KSPLIT_CASES, "w13_ragged_3_slices_of_3")[1], {"residual": True}, {**KSPLIT_KNOBS, "v10_slices": 3}, True, "v10k", ALL3),
    ("v10k_res_same_buffer", _case(KSPLIT_CASES, "w80_two_requests")[1], {"residual": True}, {**KSPLIT_KNOBS, "v10_slices": 3}, True, "v10k", SAME_BUF),
    ("strip_c64_32", _case(STRIP_CONV_CASES, "c64_32_ragged_walk7")[1], {"act": False}, {"conv_strip": 7}, True, "strip", XY),
    ("strip_c128_64_ksplit", _case(STRIP_CONV_CASES, "c128_64_ksplit_odd_rows")[1], {}, {"conv_strip": 5}, True, "strip", XY),
    ("strip_s2_odd", _case(STRIP_CONV_CASES, "c64_128_s2_odd_sizes")[1], {"act": False}, {"conv_strip": 4}, True, "strip", X_ONLY),
    ("s1x1_k16_res_all", _case(S1X1_CASES, "k16_ragged_res")[1], {"residual": True}, {"conv_1x1s": 2}, False, "s1x1", ALL3),
    ("s1x1_k16_res_same_buffer", _case(S1X1_CASES, "k16_ragged_res")[1], {"residual": True}, {"conv_1x1s": 2}, False, "s1x1", SAME_BUF),
    ("s1x1_k8_two_pixel_waves_res_only", _case(S1X1_CASES, "k8_128_64_two_pixel_waves")[1], {"residual": True}, {"conv_1x1s": 2}, False, "s1x1", RES_ONLY),
    ("s1x1_k24_x_only", _case(S1X1_CASES, "k24_384_128_sliced_noact")[1], {"act": False}, {"conv_1x1s": 2}, False, "s1x1", X_ONLY),
    ("s1x1_k2_stages_of_512", _case(S1X1_CASES, "k2_32_64_stages_of_512")[1], {"residual": True}, {"conv_1x1s": 2}, False, "s1x1", ALL3),
]


@pytest.mark.parametrize("dtype", HALVES)
@pytest.mark.parametrize("name,shape,kw,knobs,ws,variant,views", FWD_SLICED, ids=[c[0] for c in FWD_SLICED])
def test_conv_forward_on_sliced_views(dev, tune, dtype, name, shape, kw, knobs, ws, variant, views):
    """y3_conv2d_fwd(_ws), every MFMA variant, with x / the shortcut / the output as channel slices (run_conv checks poison, canary and untouched inputs): inside the
    contiguous tests' tolerance of the fp32 reference, and the bits of the pitch == c launch of the same variant"""
    for key, val in knobs.items():
        tune(key, val)
    out, ref = run_conv(dev, dtype, *shape, algo=1, ws=ws, expect=variant, repeat=2, views=views, **kw)
    flat, _ = run_conv(dev, dtype, *shape, algo=1, ws=ws, expect=variant, views={}, **kw)
    _conv_tol_check(name, dtype, out, ref)
    assert torch.equal(out, flat), f"{name} {dtype} ({variant}): sliced and contiguous launches differ, max {(out - flat).abs().max().item():.3g}"


def test_conv_direct_fp32_on_sliced_views(dev):
    """the fp32 direct kernel (64-bit indexing, no buffer descriptors) on sliced x / shortcut / output: the north-star 1e-4 of test_conv_direct_fp32_vs_reference"""
    shape = _case(CONV_CASES, "residual")[1]
    views = {"x": (4, 12), "res": (8, 16), "y": (12, 4)}   # 16-byte = 4-float slice starts
    out, ref = run_conv(dev, torch.float32, *shape, algo=2, residual=True, expect="direct", views=views)
    flat, _ = run_conv(dev, torch.float32, *shape, algo=2, residual=True, expect="direct", views={})
    err = (out - ref).abs().max().item()
    assert err < 1e-4, f"max abs err {err:.3g}"
    assert torch.equal(out, flat)


# ------------------------------------------------------------------------------------------------ statistics rows
STATS_SLICED = [
    # id, (n,h,w,cin,cout,k,s), knobs, workspace, variant
    ("v3_bk64", (2, 40, 40, 128, 256, 3, 1), {}, False, "v3_bk64_128x128"),
    ("v6_ragged_last_tile", (4, 20, 20, 512, 512, 3, 1), {}, False, "v6"),
    ("v3_64x256_odd_pixels", (2, 33, 17, 32, 64, 3, 1), {}, False, "v3_bk32_64x256"),
    ("v2_small_cin", (1, 20, 20, 16, 32, 3, 1), {}, False, "v2_smallc"),
    ("s1x1_k16", (3, 37, 29, 256, 128, 1, 1), {"conv_1x1s": 2}, False, "s1x1"),
    ("v10", (5, 20, 20, 64, 256, 3, 1), {"conv_v10": 2, "v10_blocks": 3, "v10_half": 0}, False, "v10"),
    ("v10h", (5, 20, 20, 64, 256, 3, 1), {"conv_v10": 2, "v10_blocks": 3, "v10_half": 1}, False, "v10h"),
    ("v10k", (3, 20, 19, 128, 256, 3, 1), {"v10_slices": 3}, True, "v10k"),
    ("strip", (2, 20, 64, 64, 32, 3, 1), {"conv_strip": 2}, True, "strip"),
]


@pytest.mark.parametrize("dtype", HALVES)
@pytest.mark.parametrize("name,shape,knobs,ws,variant", STATS_SLICED, ids=[c[0] for c in STATS_SLICED])
def test_conv_statistics_rows_on_sliced_views(dev, tune, dtype, name, shape, knobs, ws, variant):
    """y3_conv2d_fwd_stats(_ws) with x and the output sliced: the same rows and the same output, bit for bit, as the pitch == c launch; their fp64 sum equals the statistics of
    the stored tensor (the 1e-5 of test_conv_epilogue_bn_statistics)"""
    _lib, ops = _ops()
    for key, val in knobs.items():
        tune(key, val)
    n, h, w, cin, cout, k, s = shape
    g = torch.Generator().manual_seed(4)
    x = torch.randn(n, h, w, cin, generator=g)
    wt = torch.randn(cout, cin, k, k, generator=g) / math.sqrt(cin * k * k)
    ho, wo = (h + 2 * (k // 2) - k) // s + 1, (w + 2 * (k // 2) - k) // s + 1
    filt = ops.pack_filter(wt.to(dev), cout, cin, dtype)
    zb = torch.zeros(cout, device=dev)
    wsp = conv_ws(dev) if ws else None
    res = {}
    for form, (px, py) in (("sliced", (PX, PY)), ("flat", (None, None))):
        xb = Buf(ops, dev, dtype, (n, h, w, cin), px, NAN, x).snap()
        yb = Buf(ops, dev, dtype, (n, ho, wo, cout), py, 7.0).snap()
        rows = ops.conv2d_stats_rows(xb.v, yb.v, k, s, workspace=wsp)
        buf = torch.full((rows * 2 * cout,), NAN, device=dev)
        assert ops.conv2d_stats(xb.v, filt, zb, yb.v, k, s, buf, rows, workspace=wsp) == rows
        torch.cuda.synchronize()
        assert ops.last_conv_variant() == variant, ops.last_conv_variant()
        xb.check(f"{variant} input")
        yb.check(f"{variant} output", written=True)
        res[form] = (rows, buf.view(rows, cout, 2), yb.nhwc())
    rows, buf, y = res["sliced"]
    assert torch.isfinite(buf).all() and torch.isfinite(y.float()).all(), "a statistics row or an output pixel is not finite"
    assert rows == res["flat"][0] and torch.equal(buf, res["flat"][1]), "statistics rows of the sliced launch differ from the contiguous launch"
    assert torch.equal(y, res["flat"][2])
    u = y.double().cpu().reshape(-1, cout)
    tot = buf.double().sum(0).cpu()
    assert (tot[:, 0] - u.sum(0)).abs().max().item() <= 1e-5 * u.abs().sum(0).max().item(), "sum"
    assert (tot[:, 1] - (u * u).sum(0)).abs().max().item() <= 1e-5 * (u * u).sum(0).max().item(), "sum of squares"
    ref = F.conv2d(x.to(dtype).float().permute(0, 3, 1, 2), wt.to(dtype).float(), None, stride=s, padding=k // 2)
    _conv_tol_check(name, dtype, y.float().cpu().permute(0, 3, 1, 2), ref)


# ------------------------------------------------------------------------------------------------ BN on load, Bottleneck pair
@pytest.mark.parametrize("dtype", HALVES)
@pytest.mark.parametrize("name,shape,shortcut,silu", [_case(BNIN_CASES, "256_128_shortcut_ragged"), _case(BNIN_CASES, "128_64_plain_noact"), _case(BNIN_CASES, "128_64_shortcut")],
                         ids=["256_128_shortcut_ragged", "128_64_plain_noact", "128_64_shortcut"])
def test_conv1x1_bn_in_on_sliced_views(dev, tune, dtype, name, shape, shortcut, silu):
    """y3_conv2d_fwd_bnin_stats (conv_1x1s.h, IN form) with u_in, the shortcut, the stored normalised tensor and the output ALL channel slices: the same bits as the launch on
    pitch == c tensors, which test_conv1x1_bn_in_consumer_matches_separate_passes ties to the two launches it replaces; and the fp32 reference of the whole chain"""
    _lib, ops = _ops()
    tune("conv_1x1s", 2)
    n, h, w, cin, cout = shape
    g = torch.Generator().manual_seed(7)
    u = torch.randn(n, h, w, cin, generator=g) * 1.5
    r = torch.randn(n, h, w, cin, generator=g) if shortcut else None
    scale = (torch.rand(cin, generator=g) + 0.5).to(dev)
    shift = torch.randn(cin, generator=g).to(dev) * 0.3
    wt = torch.randn(cout, cin, 1, 1, generator=g) / math.sqrt(cin)
    filt = ops.pack_filter(wt.to(dev), cout, cin, dtype)
    zb = torch.zeros(cout, device=dev)
    act = _lib.Y3_ACT_SILU if silu else _lib.Y3_ACT_NONE
    res = {}
    for form, pads in (("sliced", (PX, PR, (24, 16), PY)), ("flat", (None,) * 4)):
        ub = Buf(ops, dev, dtype, (n, h, w, cin), pads[0], NAN, u).snap()
        rb = Buf(ops, dev, dtype, (n, h, w, cin), pads[1], NAN, r).snap() if shortcut else None
        ib = Buf(ops, dev, dtype, (n, h, w, cin), pads[2], -7.0).snap()
        ob = Buf(ops, dev, dtype, (n, h, w, cout), pads[3], -7.0).snap()
        rows = ops.conv1x1_bnin_rows(ub.v, ib.v, ob.v, shortcut)
        assert rows > 0, "the input-transform form refused this view"
        buf = torch.full((rows * 2 * cout,), NAN, device=dev)
        got = ops.conv1x1_bnin_stats(ub.v, scale, shift, act, rb.v if rb else None, ib.v, filt, zb, ob.v, buf, rows)
        torch.cuda.synchronize()
        assert got == rows and ops.last_conv_variant() == "s1x1_bn"
        ub.check("u_in")
        if rb:
            rb.check("shortcut")
        ib.check("y_in", written=True)
        ob.check("y", written=True)
        res[form] = (ib.nhwc(), ob.nhwc(), buf.view(rows, cout, 2))
    yi, yo, rows_s = res["sliced"]
    assert torch.isfinite(yi.float()).all() and torch.isfinite(yo.float()).all() and torch.isfinite(rows_s).all()
    assert torch.equal(yi, res["flat"][0]), "normalised tensor"
    assert torch.equal(yo, res["flat"][1]), "conv output"
    assert torch.equal(rows_s, res["flat"][2]), "statistics rows"
    # the chain on the rounded operands: y_in = act(scale u + shift) (+ shortcut) rounded once (the arithmetic of y3_bn_act_fwd: the 1.01 ulp of the largest value that
    # test_bn_passes_plain_and_nontemporal_forms allows it), the conv of the STORED y_in inside the conv tolerance
    z = u.to(dtype).double() * scale.cpu().double() + shift.cpu().double()
    z = z * torch.sigmoid(z) if silu else z
    if shortcut:
        z = z + r.to(dtype).double()
    ulp = 2.0 ** -10 if dtype == torch.float16 else 2.0 ** -7
    assert (yi.double().cpu() - z).abs().max().item() <= 1.01 * ulp * z.abs().max().item()
    ref = F.conv2d(yi.float().cpu().permute(0, 3, 1, 2), wt.to(dtype).float())
    _conv_tol_check(name, dtype, yo.float().cpu().permute(0, 3, 1, 2), ref)


@pytest.mark.parametrize("c", [64, 128])
@pytest.mark.parametrize("dtype", HALVES)
@pytest.mark.parametrize("name,shape,add", [_case(BNECK_CASES, "odd_rect"), _case(BNECK_CASES, "square")], ids=["odd_rect", "square"])
def test_bneck_pair_on_sliced_views(dev, dtype, name, shape, add, c):
    """y3_bneck_pair_fwd with add: x (input AND shortcut) and y as channel slices -- the reference and the bound of test_bneck_pair_vs_fp32_reference, the bits of the
    pitch == c launch"""
    _lib, ops = _ops()
    n, h, w = shape
    g = torch.Generator().manual_seed(23)
    cm = c // 2
    x = torch.randn(n, c, h, w, generator=g).to(dtype)
    w1 = (torch.randn(cm, c, 1, 1, generator=g) / math.sqrt(c)).to(dtype).float()
    b1 = torch.randn(cm, generator=g) * 0.1
    w2 = (torch.randn(c, cm, 3, 3, generator=g) / math.sqrt(9 * cm)).to(dtype).float()
    b2 = torch.randn(c, generator=g) * 0.1
    t = F.silu(F.conv2d(x.float(), w1, b1)).to(dtype).float()
    ref = F.silu(F.conv2d(t, w2, b2, padding=1)).to(dtype).float() + x.float()
    f1 = ops.pack_filter(w1.to(dev), cm, c, dtype)
    f2 = ops.pack_filter(w2.to(dev), c, cm, dtype)
    b1d, b2d = b1.to(dev), b2.to(dev)
    outs = {}
    for form, (px, py) in (("sliced", (PX, PY)), ("flat", (None, None))):
        xb = Buf(ops, dev, dtype, (n, h, w, c), px, NAN, x.permute(0, 2, 3, 1)).snap()
        yb = Buf(ops, dev, dtype, (n, h, w, c), py, 7.0).snap()
        ops.bneck_pair(xb.v, f1, b1d, True, f2, b2d, True, True, yb.v)
        torch.cuda.synchronize()
        xb.check("bneck_pair input")
        yb.check("bneck_pair output", written=True)
        outs[form] = yb.nhwc()
    got = outs["sliced"].float().cpu().permute(0, 3, 1, 2)
    assert torch.isfinite(got).all()
    tol = 2.0**-8 if dtype == torch.float16 else 2.0**-5
    err = (got - ref).abs().max().item() / ref.abs().max().item()
    assert err < tol, f"{name} {dtype}: {err:.2e}"
    assert torch.equal(outs["sliced"], outs["flat"])


def test_stem_pair_into_a_channel_slice(dev):
    """y3_stem_pair_fwd reads the NCHW image; its OUTPUT as a channel slice: canary intact, the bits of the pitch == c launch (which test_stem_pair_vs_fp32_reference ties
    to the fp32 reference), and that test's bound again"""
    _lib, ops = _ops()
    dtype = torch.float16
    n, h, w = 1, 37, 53
    g = torch.Generator().manual_seed(11)
    x = torch.rand(n, 3, h, w, generator=g).to(dtype)
    w0 = (torch.randn(32, 3, 3, 3, generator=g) / math.sqrt(27)).to(dtype).float()
    b0 = torch.randn(32, generator=g) * 0.1
    w1 = (torch.randn(64, 32, 3, 3, generator=g) / math.sqrt(288)).to(dtype).float()
    b1 = torch.randn(64, generator=g) * 0.1
    y0 = F.silu(F.conv2d(x.float(), w0, b0, stride=1, padding=1)).to(dtype).float()
    ref = F.silu(F.conv2d(y0, w1, b1, stride=2, padding=1))
    f0 = ops.pack_filter_stem(w0.to(dev), 32, dtype)
    f1 = ops.pack_filter(w1.to(dev), 64, 32, dtype)
    xd, b0d, b1d = x.to(dev), b0.to(dev), b1.to(dev)
    outs = {}
    for form, py in (("sliced", PY), ("flat", None)):
        yb = Buf(ops, dev, dtype, (n, ref.shape[2], ref.shape[3], 64), py, 7.0).snap()
        ops.stem_pair(xd, f0, b0d, True, f1, b1d, True, yb.v)
        torch.cuda.synchronize()
        yb.check("stem_pair output", written=True)
        outs[form] = yb.nhwc()
    got = outs["sliced"].float().cpu().permute(0, 3, 1, 2)
    assert (got - ref).abs().max().item() / ref.abs().max().item() < 2.0**-8
    assert torch.equal(outs["sliced"], outs["flat"])


# ------------------------------------------------------------------------------------------------ filter gradient
WGRAD_SLICED = [
    # id, (n,h,w,cin,cout,k,s), knobs, dtypes, expected tile of y3_conv2d_wgrad_plan, relative bound of the contiguous test of that plan (per dtype)
    ("tile128_3x3s1", (2, 20, 20, 64, 128, 3, 1), {"wgrad_patch": 0, "wgrad_strip": 0}, HALVES, 128, {torch.float16: 2e-3, torch.bfloat16: 1.5e-2}),
    ("tile128_3x3s2_odd", (2, 23, 19, 128, 256, 3, 2), {}, HALVES, 128, {torch.float16: 2e-3, torch.bfloat16: 1.5e-2}),
    ("tile128_1x1_deep", (2, 10, 10, 1024, 512, 1, 1), {}, HALVES, 128, {torch.float16: 2e-3, torch.bfloat16: 1.5e-2}),
    ("tile256_3x3s1_80", (4, 80, 80, 128, 256, 3, 1), {"wgrad_patch": 0}, HALVES, 256, {torch.float16: 2e-3, torch.bfloat16: 1.5e-2}),
    ("strip_c32_s1_ragged", (3, 19, 150, 32, 64, 3, 1), {"wgrad_strip": 7}, HALVES, 3, {torch.float16: 2e-5, torch.bfloat16: 2e-5}),
    ("strip_c64_s2", (2, 40, 140, 64, 128, 3, 2), {"wgrad_strip": 4}, HALVES, 3, {torch.float16: 2e-5, torch.bfloat16: 2e-5}),
    ("patch_many_slices", (7, 20, 20, 64, 128, 3, 1), {"wgrad_patch": 2}, HALVES, 4, {torch.float16: 2e-5, torch.bfloat16: 2e-5}),
    ("patch_one_slice", (1, 2, 3, 64, 128, 3, 1), {"wgrad_patch": 2}, HALVES, 4, {torch.float16: 2e-5, torch.bfloat16: 2e-5}),
    ("direct_fp32", (2, 20, 20, 64, 128, 3, 1), {}, [torch.float32], 0, {torch.float32: 2e-5}),
    ("direct_fp32_first_layer", (2, 40, 36, 8, 32, 3, 1), {}, [torch.float32], 0, {torch.float32: 2e-5}),
]
# the contiguous tests of the 128 / 256 tiles bound the error of dW computed from ROUNDED x and du against fp32 autograd on the same rounded operands by 2e-3 / 1.5e-2 of the
# largest entry, the strip / patch tests by 2e-5 (fp32 accumulation order only); the same operands and bounds here
WGRAD_PATCH_SLICES = {"patch_many_slices": lambda s: s > 1, "patch_one_slice": lambda s: s == 1}


@pytest.mark.parametrize("name,shape,knobs,dtype,tile,bound", [(c[0], c[1], c[2], dt, c[4], c[5][dt]) for c in WGRAD_SLICED for dt in c[3]],
                         ids=[f"{c[0]}-{str(dt).split('.')[-1]}" for c in WGRAD_SLICED for dt in c[3]])
def test_conv_wgrad_on_sliced_views(dev, tune, name, shape, knobs, dtype, tile, bound):
    """y3_conv2d_wgrad on every plan with x AND du channel slices of NaN-filled buffers: dW and the bias gradient are finite, within the plan's own bound of fp32 autograd on the
    same rounded operands, and the bits of the launch on pitch == c tensors (same plan: tile, slices, grouping); x and du are not written.  The form that RAN is asserted
    (y3_conv2d_wgrad_last_plan): the dry run's, except that the strip kernel refuses a bias gradient -- those launches take what the dry run plans with wgrad_strip = 0, and
    the strip cases launch once more without a bias gradient, with the same checks on dW"""
    _lib, ops = _ops()
    for key, val in knobs.items():
        tune(key, val)
    n, h, w, cin, cout, k, s = shape
    g = torch.Generator().manual_seed(5)
    x = torch.randn(n, cin, h, w, generator=g).to(dtype).float()
    wt = torch.zeros(cout, cin, k, k, requires_grad=True)
    y = F.conv2d(x, wt, None, stride=s, padding=k // 2)
    gy = torch.randn(y.shape, generator=g).to(dtype).float()
    y.backward(gy)
    ho, wo = y.shape[2], y.shape[3]
    lp = (4, 12) if dtype == torch.float32 else PX
    rp = (8, 16) if dtype == torch.float32 else PR
    res, strip = {}, {}
    for form, (px, pg) in (("sliced", (lp, rp)), ("flat", (None, None))):
        xb = Buf(ops, dev, dtype, (n, h, w, cin), px, NAN, x.permute(0, 2, 3, 1)).snap()
        gb = Buf(ops, dev, dtype, (n, ho, wo, cout), pg, NAN, gy.permute(0, 2, 3, 1)).snap()
        plan = ops.conv2d_wgrad_plan(xb.v, cout, k, s)
        dw, db = ops.conv2d_wgrad(xb.v, gb.v, k, s, cout, cin, want_bias=True)
        launched = ops.conv2d_wgrad_last_plan()
        torch.cuda.synchronize()
        xb.check("wgrad x")
        gb.check("wgrad du")
        res[form] = (plan, dw.clone(), db.clone())
        if tile == 3:
            tune("wgrad_strip", 0)
            without_strip = ops.conv2d_wgrad_plan(xb.v, cout, k, s)
            tune("wgrad_strip", knobs["wgrad_strip"])
            assert launched == without_strip and launched[0] != 3, f"the launch with a bias gradient took {launched}, without the strip kernel the library plans {without_strip}"
            dw_s, _ = ops.conv2d_wgrad(xb.v, gb.v, k, s, cout, cin, want_bias=False)
            assert ops.conv2d_wgrad_last_plan() == plan, f"the launch without a bias gradient took {ops.conv2d_wgrad_last_plan()}, planned {plan}"
            torch.cuda.synchronize()
            xb.check("strip wgrad x")
            gb.check("strip wgrad du")
            strip[form] = dw_s.clone()
        else:
            assert launched == plan, f"the launch took {launched}, planned {plan}"
    plan, dw, db = res["sliced"]
    assert plan[0] == tile, f"the library plans tile {plan[0]} for this view, the case is written for {tile}"
    assert plan == res["flat"][0], f"sliced plan {plan} differs from the contiguous plan {res['flat'][0]}"
    if name in WGRAD_PATCH_SLICES:
        assert WGRAD_PATCH_SLICES[name](plan[1]), plan
    assert torch.isfinite(dw).all() and torch.isfinite(db).all(), "the filter gradient read poisoned memory outside its slices"
    e_w = (dw.cpu() - wt.grad).abs().max().item() / wt.grad.abs().max().item()
    e_b = (db.cpu() - gy.sum((0, 2, 3))).abs().max().item() / gy.sum((0, 2, 3)).abs().max().item()
    print(f"[wgrad views {name} {dtype}] plan {plan}: dW {e_w:.2e}, bias {e_b:.2e}")
    assert e_w < bound and e_b < max(bound, 2e-3), f"{name} {dtype}: wgrad {e_w:.2e} bias {e_b:.2e}"   # (bias bound: test_conv_wgrad_and_dgrad_vs_autograd)
    assert torch.equal(dw, res["flat"][1]) and torch.equal(db, res["flat"][2]), "sliced and contiguous filter gradients differ"
    if tile == 3:   # the strip kernel itself (no bias gradient) on pitch != c
        assert torch.isfinite(strip["sliced"]).all(), "the strip kernel read poisoned memory outside its slices"
        e_s = (strip["sliced"].cpu() - wt.grad).abs().max().item() / wt.grad.abs().max().item()
        print(f"[wgrad views {name} {dtype}] strip launch, plan {plan}: dW {e_s:.2e}")
        assert e_s < bound, f"{name} {dtype}: strip wgrad {e_s:.2e}"
        assert torch.equal(strip["sliced"], strip["flat"]), "sliced and contiguous filter gradients of the strip kernel differ"


WGRAD_FORMS = [
    # id, the smallest (n,h,w,cin,cout,k,s) that reaches the form, its knobs, dtypes, tile of the dry run, the knob that takes the form away where it refuses a request
    ("strip", (1, 3, 70, 32, 64, 3, 1), {"wgrad_strip": 7}, HALVES, 3, "wgrad_strip"),   # (refuses a bias gradient and real channel subsets)
    ("patch", (1, 2, 3, 64, 128, 3, 1), {"wgrad_patch": 2}, HALVES, 4, None),
    ("tile256", (1, 16, 16, 128, 256, 3, 1), {"wgrad": 3, "wgrad_patch": 0}, HALVES, 256, None),
    ("tile128", (2, 20, 20, 64, 128, 3, 1), {"wgrad_patch": 0, "wgrad_strip": 0}, HALVES, 128, None),
    ("direct_fp32", (2, 8, 8, 8, 32, 3, 1), {}, [torch.float32], 0, None),
]


def _wgrad_form_bound(tile, dtype):
    """the bounds of WGRAD_SLICED, by the form that ran: the tile kernels 2e-3 / 1.5e-2, strip / patch / direct 2e-5"""
    return {torch.float16: 2e-3, torch.bfloat16: 1.5e-2}[dtype] if tile in (128, 256) else 2e-5


@pytest.mark.parametrize("name,shape,knobs,dtype,tile,refusing", [(c[0], c[1], c[2], dt, c[4], c[5]) for c in WGRAD_FORMS for dt in c[3]],
                         ids=[f"{c[0]}-{str(dt).split('.')[-1]}" for c in WGRAD_FORMS for dt in c[3]])
def test_conv_wgrad_launches_the_planned_form(dev, tune, name, shape, knobs, dtype, tile, refusing):
    """every form of the filter-gradient dispatch, launched plain, with a bias gradient and with cout_real = cout - 1 on sliced x and du: the form that ran
    (y3_conv2d_wgrad_last_plan) is the dry run's -- where the form refuses the request (strip: bias gradient, real subset) the dry run's with that form's knob at 0 --
    and dW / the bias gradient are within the bound of the form that ran of fp32 autograd on the same rounded operands"""
    _lib, ops = _ops()
    for key, val in knobs.items():
        tune(key, val)
    n, h, w, cin, cout, k, s = shape
    g = torch.Generator().manual_seed(7)
    x = torch.randn(n, cin, h, w, generator=g).to(dtype).float()
    wt = torch.zeros(cout, cin, k, k, requires_grad=True)
    y = F.conv2d(x, wt, None, stride=s, padding=k // 2)
    gy = torch.randn(y.shape, generator=g).to(dtype).float()
    y.backward(gy)
    xb = Buf(ops, dev, dtype, (n, h, w, cin), (4, 12) if dtype == torch.float32 else PX, NAN, x.permute(0, 2, 3, 1)).snap()
    gb = Buf(ops, dev, dtype, (n, y.shape[2], y.shape[3], cout), (8, 16) if dtype == torch.float32 else PR, NAN, gy.permute(0, 2, 3, 1)).snap()
    plan = ops.conv2d_wgrad_plan(xb.v, cout, k, s)
    assert plan[0] == tile, f"the library plans tile {plan[0]} for this view, the case is written for {tile}"
    fallback = plan
    if refusing:
        tune(refusing, 0)
        fallback = ops.conv2d_wgrad_plan(xb.v, cout, k, s)
        tune(refusing, knobs[refusing])
        assert fallback[0] != tile
    scale = wt.grad.abs().max().item()
    for what, cout_real, want_bias, want in (("plain", cout, False, plan), ("bias", cout, True, fallback), ("real_subset", cout - 1, False, fallback)):
        dw, db = ops.conv2d_wgrad(xb.v, gb.v, k, s, cout_real, cin, want_bias=want_bias)
        launched = ops.conv2d_wgrad_last_plan()
        torch.cuda.synchronize()
        xb.check(f"wgrad x ({what})")
        gb.check(f"wgrad du ({what})")
        assert launched == want, f"{name} {what}: the launch took {launched}, expected {want} (dry run {plan})"
        bound = _wgrad_form_bound(launched[0], dtype)
        assert dw.shape[0] == cout_real and torch.isfinite(dw).all()
        e_w = (dw.cpu() - wt.grad[:cout_real]).abs().max().item() / scale
        e_b = (db.cpu() - gy.sum((0, 2, 3))).abs().max().item() / gy.sum((0, 2, 3)).abs().max().item() if want_bias else 0.0
        print(f"[wgrad forms {name} {dtype} {what}] launched {launched}: dW {e_w:.2e}, bias {e_b:.2e}")
        assert e_w < bound and e_b < max(bound, 2e-3), f"{name} {dtype} {what}: wgrad {e_w:.2e} bias {e_b:.2e}"   # (bias bound: test_conv_wgrad_and_dgrad_vs_autograd)


# ------------------------------------------------------------------------------------------------ data gradient
DGRAD_SLICED = [
    # id, (n,h,w,cin,cout,k,s)
    ("3x3s1", (2, 20, 20, 64, 128, 3, 1)),
    ("3x3s2_odd", (2, 23, 19, 128, 256, 3, 2)),
    ("1x1_deep", (2, 10, 10, 1024, 512, 1, 1)),
    ("head_255_of_256", (2, 20, 20, 64, 256, 1, 1)),
]


def _dgrad_operands(dtype, shape, seed, cout_real=None):
    n, h, w, cin, cout, k, s = shape
    cout_real = cout_real or cout
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, cin, h, w, generator=g).to(dtype).float().requires_grad_(True)
    wt = (torch.randn(cout_real, cin, k, k, generator=g) / math.sqrt(cin * k * k)).to(dtype).float()
    y = F.conv2d(x, wt, None, stride=s, padding=k // 2)
    gy = torch.randn(y.shape, generator=g).to(dtype).float()
    y.backward(gy)
    return wt, gy, x.grad


@pytest.mark.parametrize("dtype", HALVES)
@pytest.mark.parametrize("name,shape", DGRAD_SLICED, ids=[c[0] for c in DGRAD_SLICED])
def test_conv_dgrad_accumulate_on_sliced_views(dev, dtype, name, shape):
    """the data gradient through y3_conv2d_fwd on the flipped bank (dilated input for stride 2) with residual == gx (accumulate), du and gx channel slices: launched twice onto a
    zeroed gx -- once and twice the gradient inside the bounds of test_conv_wgrad_and_dgrad_vs_autograd (tol, 2 tol) -- the bits of the pitch == c launches, neighbours intact.
    head_255_of_256: 255 real filters in 256 channels of du (a Detect head) -- the pad channel of du is zero as y3_detect_raw_bwd leaves it."""
    _lib, ops = _ops()
    n, h, w, cin, cout, k, s = shape
    cout_real = 255 if name == "head_255_of_256" else cout
    wt, gy, gx_ref = _dgrad_operands(dtype, shape, 3, cout_real)
    ho, wo = gy.shape[2], gy.shape[3]
    filt_d = ops.pack_filter_dgrad(wt.to(dev), cout, cin, dtype)
    zb = torch.zeros(cin, device=dev)
    gyp = torch.zeros(n, ho, wo, cout)
    gyp[..., :cout_real] = gy.permute(0, 2, 3, 1)
    res = {}
    for form, (pg, px) in (("sliced", (PR, PX)), ("flat", (None, None))):
        gb = Buf(ops, dev, dtype, (n, ho, wo, cout), pg, NAN, gyp).snap()
        xb = Buf(ops, dev, dtype, (n, h, w, cin), px, 7.0, torch.zeros(n, h, w, cin)).snap()
        outs, variants = [], []
        for _ in range(2):
            ops.conv2d(gb.v, filt_d, zb, xb.v, k, 1, act=False, residual=xb.v, in_dilation=s)
            torch.cuda.synchronize()
            variants.append(ops.last_conv_variant())
            outs.append(xb.nhwc())
        gb.check("dgrad du")
        xb.check("dgrad gx", written=True)
        res[form] = (outs, variants)
    outs, variants = res["sliced"]
    assert variants == res["flat"][1], f"sliced launches took {variants}, contiguous {res['flat'][1]}"
    tol = {torch.float16: 2e-3, torch.bfloat16: 1.5e-2}[dtype]
    for i, o in enumerate(outs):
        assert torch.isfinite(o.float()).all()
        e = (o.float().cpu().permute(0, 3, 1, 2) - (i + 1) * gx_ref).abs().max().item() / gx_ref.abs().max().item()
        assert e < (i + 1) * tol, f"{name} {dtype} launch {i} ({variants[i]}): {e:.2e}"
        assert torch.equal(o, res["flat"][0][i]), f"launch {i} ({variants[i]}): sliced and contiguous differ"


DGRAD_S2_SLICED = [
    # id, (n,h,w,cin,cout), knobs, variant of the write launch (None: the per-class launches, whatever tile they take)
    ("v3_quad_even_cin32", (2, 32, 48, 32, 64), {"conv_strip": 0}, "v3_quad"),
    ("v3_quad_even_cin128", (2, 64, 64, 128, 256), {}, "v3_quad"),
    ("per_class_odd", (2, 23, 19, 128, 256), {}, None),
    ("strip_quad_c32_64", (3, 38, 300, 32, 64), {"conv_strip": 7}, "strip_quad"),
    ("strip_quad_c64_128", (2, 40, 128, 64, 128), {"conv_strip": 2}, "strip_quad"),
]


@pytest.mark.parametrize("dtype", HALVES)
@pytest.mark.parametrize("name,shape,knobs,variant", DGRAD_S2_SLICED, ids=[c[0] for c in DGRAD_S2_SLICED])
def test_conv_dgrad_s2_on_sliced_views(dev, tune, dtype, name, shape, knobs, variant):
    """y3_conv2d_dgrad_s2 (parity classes) with du a slice and gx -- output AND residual -- a slice: write, then accumulate; the bounds of the contiguous tests (tol for the
    write, 2 tol for write + accumulate), the bits of the pitch == c launches, same variants"""
    _lib, ops = _ops()
    for key, val in knobs.items():
        tune(key, val)
    n, h, w, cin, cout = shape
    wt, gy, gx_ref = _dgrad_operands(dtype, (n, h, w, cin, cout, 3, 2), 7)
    ho, wo = gy.shape[2], gy.shape[3]
    res = {}
    for form, (pg, px) in (("sliced", (PR, PX)), ("flat", (None, None))):
        gb = Buf(ops, dev, dtype, (n, ho, wo, cout), pg, NAN, gy.permute(0, 2, 3, 1)).snap()
        xb = Buf(ops, dev, dtype, (n, h, w, cin), px, NAN)
        xb.v.as_nhwc().fill_(NAN)   # the write form must not read it
        xb.snap()
        outs, variants = [], []
        for acc in (False, True):
            ops.conv2d_dgrad_s2(wt.to(dev), gb.v, xb.v, accumulate=acc)
            torch.cuda.synchronize()
            variants.append(ops.last_conv_variant())
            outs.append(xb.nhwc())
        gb.check("dgrad_s2 du")
        xb.check("dgrad_s2 gx", written=True)
        res[form] = (outs, variants)
    outs, variants = res["sliced"]
    assert variants == res["flat"][1], f"sliced launches took {variants}, contiguous {res['flat'][1]}"
    if variant is not None:
        assert variants[0] == variant, variants
    tol = {torch.float16: 2e-3, torch.bfloat16: 1.5e-2}[dtype]
    for i, o in enumerate(outs):
        assert torch.isfinite(o.float()).all(), f"launch {i} ({variants[i]}) left or read non-finite values"
        e = (o.float().cpu().permute(0, 3, 1, 2) - (i + 1) * gx_ref).abs().max().item() / gx_ref.abs().max().item()
        assert e < (i + 1) * tol, f"{name} {dtype} launch {i} ({variants[i]}): {e:.2e}"
        assert torch.equal(o, res["flat"][0][i]), f"launch {i} ({variants[i]}): sliced and contiguous differ"


# ------------------------------------------------------------------------------------------------ BatchNorm passes
def _bn_run(ops, _lib, dev, dtype, shape, act, residual, gres_acc, sliced, split):
    """statistics + finalize, normalise (+ residual), backward (+ residual gradient) on one set of operands; split: the backward as y3_bn_act_bwd_reduce + y3_bn_act_bwd_apply"""
    n, h, w, c = shape
    g = torch.Generator(device=dev).manual_seed(3)
    u = torch.empty(n, h, w, c, device=dev).normal_(generator=g).mul_(1.5).add_(0.25)
    dy = torch.empty(n, h, w, c, device=dev).normal_(generator=g)
    r = torch.empty(n, h, w, c, device=dev).normal_(generator=g)
    gamma = torch.rand(c, device=dev, generator=g) + 0.5
    beta = torch.randn(c, device=dev, generator=g) * 0.3
    pads = [PX, PR, PY, (24, 16), (8, 8), (40, 16)] if sliced else [None] * 6
    ub = Buf(ops, dev, dtype, shape, pads[0], NAN, u).snap()
    rb = Buf(ops, dev, dtype, shape, pads[1], NAN, r).snap() if residual else None
    yb = Buf(ops, dev, dtype, shape, pads[2], 7.0).snap()
    dyb = Buf(ops, dev, dtype, shape, pads[3], NAN, dy).snap()
    dub = Buf(ops, dev, dtype, shape, pads[4], 7.0).snap()
    grb = None
    if residual:
        grb = Buf(ops, dev, dtype, shape, pads[5], 7.0)
        grb.v.as_nhwc().fill_(0.5 if gres_acc else NAN)   # (the write form must not read it)
        grb.snap()
    sums = ops.bn_scratch(c, dev)
    scale, shift, mean, invstd, dgamma, dbeta = (torch.full((c,), NAN, device=dev) for _ in range(6))
    rmean, rvar = torch.zeros(c, device=dev), torch.ones(c, device=dev)
    v, a, gres = ops.BnVecs(scale, shift, mean, invstd, sums), (_lib.Y3_ACT_SILU if act else _lib.Y3_ACT_NONE), (grb.v if grb else None)
    ops.bn_stats_finalize(ub.v, ops.bn_affine(gamma, beta, 1e-3, 0.03, rmean, rvar), v)
    ops.bn_act_fwd(ub.v, v, a, yb.v, rb.v if rb else None)
    if split:
        ops.bn_act_bwd_reduce(ub.v, dyb.v, v, a, dgamma, dbeta)
        ops.bn_act_bwd_apply(ub.v, dyb.v, v, a, dub.v, gres, gres_acc)
    else:
        ops.bn_act_bwd(ub.v, dyb.v, v, a, dub.v, dgamma, dbeta, gres, gres_acc)
    torch.cuda.synchronize()
    ub.check("bn u")
    dyb.check("bn dy")
    if rb:
        rb.check("bn residual")
    yb.check("bn y", written=True)
    dub.check("bn du", written=True)
    if grb:
        grb.check("bn gres", written=True)
    out = dict(y=yb.nhwc(), du=dub.nhwc(), dgamma=dgamma, dbeta=dbeta, mean=mean, invstd=invstd, rmean=rmean, rvar=rvar, scale=scale, shift=shift)
    if grb:
        out["gres"] = grb.nhwc()
    ops_in = dict(u=ub.nhwc(), dy=dyb.nhwc(), r=rb.nhwc() if rb else None, gamma=gamma, beta=beta)
    return out, ops_in


BN_SLICED = [
    # id, (n,h,w,c), SiLU, residual
    ("c128_res", (2, 40, 40, 128), True, True),
    ("c64_ragged", (3, 23, 19, 64), True, False),
    ("c256_linear", (1, 64, 64, 256), False, False),
    ("c1024_res_linear", (2, 16, 16, 1024), False, True),
]


@pytest.mark.parametrize("dtype", HALVES)
@pytest.mark.parametrize("nt", [0, 1], ids=["plain", "nontemporal"])
@pytest.mark.parametrize("name,shape,act,residual,gres_acc", [c + (acc,) for c in BN_SLICED for acc in ((0, 1) if c[3] else (0,))],
                         ids=[c[0] + ("_gres_accumulate" if acc else "") for c in BN_SLICED for acc in ((0, 1) if c[3] else (0,))])
def test_bn_passes_on_sliced_views(dev, tune, dtype, nt, name, shape, act, residual, gres_acc):
    """y3_bn_stats_finalize, y3_bn_act_fwd, y3_bn_act_bwd / y3_bn_act_bwd_res with u, the residual, y, dy, du and the residual's gradient ALL channel slices (six different
    paddings), plain and non-temporal forms, the residual gradient written and accumulated: the fp64 reference and the bounds of test_bn_passes_plain_and_nontemporal_forms, the
    bits of the pitch == c launches, and -- the header's promise -- y3_bn_act_bwd_reduce + y3_bn_act_bwd_apply back to back give the bits of y3_bn_act_bwd(_res), on sliced and
    on contiguous views."""
    _lib, ops = _ops()
    tune("bn_nt_bytes", 0 if nt else 1 << 62)
    n, h, w, c = shape
    M = n * h * w
    o, src = _bn_run(ops, _lib, dev, dtype, shape, act, residual, gres_acc, sliced=True, split=False)
    yr, dur, dgr, dbr, mr, vr = _bn_reference(src["u"].view(M, c), src["dy"].view(M, c), src["gamma"], src["beta"], 1e-3, act, src["r"].view(M, c) if residual else None)
    ulp = 2.0 ** -10 if dtype == torch.float16 else 2.0 ** -7
    for k_, v in o.items():
        assert torch.isfinite(v.float()).all(), f"{k_} is not finite: a pass read outside its slices"
    dysum = src["dy"].float().abs().sum().item()
    assert (o["mean"].double() - mr).abs().max().item() <= 1e-5 * max(1.0, mr.abs().max().item())
    assert (o["invstd"].double() - 1 / torch.sqrt(vr + 1e-3)).abs().max().item() <= 1e-5 * o["invstd"].max().item()
    assert (o["rmean"].double() - 0.03 * mr).abs().max().item() <= 1e-6 + 1e-5 * mr.abs().max().item()
    assert (o["rvar"].double() - (0.97 + 0.03 * vr * M / (M - 1))).abs().max().item() <= 1e-5
    assert (o["y"].view(M, c).double() - yr).abs().max().item() <= 1.01 * ulp * yr.abs().max().item()
    assert (o["du"].view(M, c).double() - dur).abs().max().item() <= 1.5 * ulp * dur.abs().max().item() + 1e-6
    assert (o["dgamma"].double() - dgr).abs().max().item() <= 2e-5 * dysum / c
    assert (o["dbeta"].double() - dbr).abs().max().item() <= 2e-5 * dysum / c
    if residual:
        want = (0.5 + src["dy"].float()).to(dtype) if gres_acc else src["dy"]
        assert torch.equal(o["gres"], want), "residual gradient"
    for sliced, split in ((False, False), (True, True), (False, True)):
        o2, _ = _bn_run(ops, _lib, dev, dtype, shape, act, residual, gres_acc, sliced=sliced, split=split)
        for k_ in o:
            assert torch.equal(bits(o[k_]), bits(o2[k_])), f"{k_}: sliced one-call form differs from the {'sliced' if sliced else 'contiguous'} {'reduce + apply' if split else 'one-call'} form"


@pytest.mark.parametrize("n_rows", [37, 512, 600, 5000])
def test_bn_sum_rows_and_devcount_equal_finalize_rows(dev, n_rows):
    """y3_bn_sum_rows + y3_bn_finalize_devcount (the SyncBatchNorm forward of one rank) against y3_bn_finalize_rows with the host count: scale, shift, mean, invstd and the running
    statistics bit for bit -- one level (<= 512 rows) and two levels of the row sum"""
    _lib, ops = _ops()
    c, count = 136, 64 * n_rows - 5
    g = torch.Generator().manual_seed(n_rows)
    rows = torch.empty(n_rows, c, 2)
    rows[..., 0] = torch.randn(n_rows, c, generator=g) * 8
    rows[..., 1] = torch.rand(n_rows, c, generator=g) * 200 + 64
    rows = rows.to(dev)
    gamma, beta = (torch.rand(c, generator=g) + 0.5).to(dev), torch.randn(c, generator=g).to(dev)
    outs = []
    for form in ("rows", "devcount"):
        sums = ops.bn_scratch(c, dev)
        rm, rv = torch.full((c,), 0.25, device=dev), torch.full((c,), 1.5, device=dev)
        scale, shift, mean, invstd = (torch.full((c,), NAN, device=dev) for _ in range(4))
        affine, v = ops.bn_affine(gamma, beta, 1e-3, 0.03, rm, rv), ops.BnVecs(scale, shift, mean, invstd, sums)
        if form == "rows":
            ops.bn_finalize_rows(rows, n_rows, count, c, affine, v)
        else:
            cnt = torch.tensor([float(count)], dtype=torch.float64, device=dev)
            ops.bn_sum_rows(rows, n_rows, c, sums)
            ops.bn_finalize_devcount(cnt, c, affine, v)
        torch.cuda.synchronize()
        outs.append(dict(scale=scale, shift=shift, mean=mean, invstd=invstd, rmean=rm, rvar=rv, totals=sums[: 2 * c].clone()))
    for k_ in outs[0]:
        assert torch.isfinite(outs[0][k_]).all(), k_
        assert torch.equal(outs[0][k_], outs[1][k_]), f"{k_}: sum_rows + finalize_devcount differs from finalize_rows"
    # and the totals are the sums of the rows: both sides add <= 5000 fp32 values in fp64, each add off by <= 2^-53 of the absolute sum -- 2 x 5000 x 2^-53 < 1.2e-12
    tot = rows.double().sum(0).reshape(-1).cpu()
    assert (outs[0]["totals"].cpu() - tot).abs().max().item() <= 1.2e-12 * rows.double().abs().sum(0).max().item()


# ------------------------------------------------------------------------------------------------ max-pool backward (SPP), stem backward
@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
@pytest.mark.parametrize("k", [5, 9, 13])
def test_maxpool_backward_on_a_slice_of_the_spp_gradient(dev, dtype, k):
    """SPPPoolUnit.bwd: dy = slice j of the 3C-channel pyramid gradient, x and dx slices of other buffers; y3_maxpool2d_bwd (gather) and y3_maxpool2d_bwd_ws (indexed), write
    then accumulate: the bits of the pitch == c launches, both forms the same bits, and -- fp32, tie-free -- torch's max_pool2d autograd (the 1e-6 of
    test_maxpool_backward_indexed_form)"""
    _lib, ops = _ops()
    n, h, w, c = 3, 11, 17, 40
    j = (5, 9, 13).index(k)
    g = torch.Generator().manual_seed(23)
    xt = torch.randn(n, c, h, w, generator=g).to(dtype).float()
    gy3 = torch.randn(n, h, w, 3 * c, generator=g).to(dtype).float()
    gy = gy3[..., j * c : (j + 1) * c]
    vec = 4 if dtype == torch.float32 else 8
    res = {}
    for form in ("gather", "indexed"):
        for layout in ("sliced", "flat"):
            sl = layout == "sliced"
            xb = Buf(ops, dev, dtype, (n, h, w, c), (2 * vec, 3 * c) if sl else None, NAN, xt.permute(0, 2, 3, 1)).snap()   # cv1's output: the first slice of SPP's concat buffer
            if sl:
                pyr = Buf(ops, dev, dtype, (n, h, w, 3 * c), (2 * vec, 2 * vec), NAN, gy3).snap()
                gv = pyr.v.slice(j * c, c)
            else:
                pyr = Buf(ops, dev, dtype, (n, h, w, c), None, NAN, gy).snap()
                gv = pyr.v
            if sl:   # the other two slices of the pyramid gradient are not this launch's business either
                pyr.v.as_nhwc()[..., : j * c] = NAN
                pyr.v.as_nhwc()[..., (j + 1) * c :] = NAN
                pyr.snap()
            db = Buf(ops, dev, dtype, (n, h, w, c), (vec, 5 * vec) if sl else None, 7.0)
            db.v.as_nhwc().fill_(NAN)
            db.snap()
            outs = []
            for acc in (False, True):
                if form == "gather":
                    ops.maxpool2d_bwd_gather(xb.v, gv, db.v, k, 1, k // 2, accumulate=acc)
                else:
                    ops.maxpool2d_bwd(xb.v, gv, db.v, k, 1, k // 2, accumulate=acc)
                torch.cuda.synchronize()
                outs.append(db.nhwc())
            xb.check("maxpool x")
            pyr.check("maxpool dy")
            db.check("maxpool dx", written=True)
            res[form, layout] = outs
    for i in range(2):
        first = res["gather", "sliced"][i]
        assert torch.isfinite(first.float()).all()
        for key, outs in res.items():
            assert torch.equal(first, outs[i]), f"{'accumulate' if i else 'write'}: {key} differs from (gather, sliced)"
    if dtype == torch.float32:
        xr = xt.clone().requires_grad_(True)
        F.max_pool2d(xr, k, 1, k // 2).backward(gy.permute(0, 3, 1, 2).contiguous())
        torch.testing.assert_close(res["indexed", "sliced"][0].cpu().permute(0, 3, 1, 2), xr.grad, rtol=1e-6, atol=1e-6)
        torch.testing.assert_close(res["indexed", "sliced"][1].cpu().permute(0, 3, 1, 2), 2 * xr.grad, rtol=1e-6, atol=1e-6)


@pytest.mark.parametrize("dtype", HALVES)
@pytest.mark.parametrize("shape,act", [((2, 3, 40, 72), True), ((1, 3, 37, 131), True), ((2, 1, 19, 64), False)], ids=["l0", "ragged", "cin1_noact"])
def test_stem_bn_bwd_wgrad_on_sliced_views(dev, dtype, shape, act):
    """y3_stem_bn_bwd_wgrad with u and dy channel slices: dgamma, dbeta and dW are the bits of the pitch == c launch; dgamma / dbeta the bits of y3_bn_act_bwd and dW within
    2e-5 of the unfused path (the bounds of test_stem_bn_bwd_wgrad_matches_unfused_backward); u and dy are not written"""
    _lib, ops = _ops()
    n, cin, h, w = shape
    cout = 32
    g = torch.Generator().manual_seed(17)
    x = torch.rand(n, cin, h, w, generator=g).to(torch.float16)
    xd = x.to(dev)
    u = (torch.randn(n, h, w, cout, generator=g) * 1.5).to(dtype)
    dy = (torch.randn(n, h, w, cout, generator=g) * 0.1).to(dtype)
    gamma, beta = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g) * 0.1
    uf = u.double()
    mean = uf.mean((0, 1, 2))
    invstd = 1.0 / torch.sqrt(uf.var((0, 1, 2), unbiased=False) + 1e-3)
    scale = (gamma.double() * invstd).float().to(dev)
    shift = (beta.double() - mean * gamma.double() * invstd).float().to(dev)
    mean_d, invstd_d = mean.float().to(dev), invstd.float().to(dev)
    a = _lib.Y3_ACT_SILU if act else _lib.Y3_ACT_NONE
    res = {}
    for form, (pu, pg) in (("sliced", (PX, PR)), ("flat", (None, None))):
        ub = Buf(ops, dev, dtype, (n, h, w, cout), pu, NAN, u).snap()
        gb = Buf(ops, dev, dtype, (n, h, w, cout), pg, NAN, dy).snap()
        sums = ops.bn_scratch(cout, dev)
        dg, db_ = torch.full((cout,), NAN, device=dev), torch.full((cout,), NAN, device=dev)
        dw = torch.full((cout, cin, 3, 3), NAN, device=dev)
        ops.stem_bn_bwd_wgrad(xd, ub.v, gb.v, scale, shift, mean_d, invstd_d, a, sums, dg, db_, dw, ops.stem_bwd_workspace(dev))
        torch.cuda.synchronize()
        ub.check("stem backward u")
        gb.check("stem backward dy")
        res[form] = (dg, db_, dw, ub, gb)
    dg, db_, dw, ub, gb = res["sliced"]
    assert torch.isfinite(dg).all() and torch.isfinite(db_).all() and torch.isfinite(dw).all()
    for i, what in enumerate(("dgamma", "dbeta", "dW")):
        assert torch.equal(res["sliced"][i], res["flat"][i]), f"{what}: sliced and contiguous differ"
    # the unfused path on the same (sliced) operands: du stored, generic filter gradient
    sums = ops.bn_scratch(cout, dev)
    duv = ops.View.alloc(n, h, w, cout, dtype, dev)
    dg0, db0 = torch.empty(cout, device=dev), torch.empty(cout, device=dev)
    ops.bn_act_bwd(ub.v, gb.v, ops.BnVecs(scale, shift, mean_d, invstd_d, sums), a, duv, dg0, db0)
    xin = ops.View.alloc(n, h, w, 8, dtype, dev)
    ops.nchw_to_nhwc(xd, xin)
    dw0, _ = ops.conv2d_wgrad(xin, duv, 3, 1, cout, cin)
    torch.cuda.synchronize()
    assert torch.equal(dg0, dg) and torch.equal(db0, db_)
    ref = dw0.abs().max().item()
    assert (dw0 - dw).abs().max().item() <= 2e-5 * ref + 1e-6, f"fused vs unfused dW: {(dw0 - dw).abs().max().item():.3e} of {ref:.3e}"


# ------------------------------------------------------------------------------------------------ exports no other test calls directly
def _ulp(t, dtype):
    """one unit in the last place of `dtype` at the magnitude of each element of t (fp64); the subnormal spacing below the smallest normal"""
    mant, emin = {torch.float16: (10, -14), torch.bfloat16: (7, -126), torch.float32: (23, -126)}[dtype]
    e = torch.floor(torch.log2(t.abs().clamp_min(2.0 ** emin)))
    return torch.pow(2.0, e - mant)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float32])
@pytest.mark.parametrize("accumulate", [0, 1], ids=["write", "accumulate"])
@pytest.mark.parametrize("shape", [(2, 13, 7, 40), (1, 5, 9, 136), (3, 10, 10, 256)], ids=["odd_c40", "odd_c136", "c256"])
def test_upsample2x_bwd(dev, dtype, accumulate, shape):
    """y3_upsample2x_bwd: dx (+)= the 2x2 block of dy.  Reference: the fp64 sum of the four taps (plus the old dx when accumulating) rounded ONCE to the storage type.
    Bound, halves: the kernel (csrc/train.hip upsample2x_bwd_kernel) loads the old dx and the four taps into fp32, adds them in fp32 and rounds once on the store -- also when
    accumulating, so one rounding, not two: one ulp of the storage type at the result's magnitude (the fp32 sum of <= five 11-bit values is exact or off by < 2^-13 ulp of the
    half, which can at most flip the final rounding to the neighbouring value).  fp32: every add rounds; 3 adds (4 when accumulating) of error <= 2^-24 |partial sum| each
    plus the reference's own rounding: (adds + 1) 2^-24 sum |terms|.  On contiguous and on sliced views (poison / canary), sliced == contiguous bit for bit."""
    _lib, ops = _ops()
    n, h, w, c = shape
    g = torch.Generator().manual_seed(31)
    dy = torch.randn(n, 2 * h, 2 * w, c, generator=g).to(dtype)
    old = torch.randn(n, h, w, c, generator=g).to(dtype)
    taps = dy.double().view(n, h, 2, w, 2, c)
    ref = taps.sum((2, 4)) + (old.double() if accumulate else 0.0)
    mag = taps.abs().sum((2, 4)) + (old.double().abs() if accumulate else 0.0)
    vec = 4 if dtype == torch.float32 else 8
    outs = {}
    for form, (pg, px) in (("sliced", ((2 * vec, 4 * vec), (4 * vec, 2 * vec))), ("flat", (None, None))):
        gb = Buf(ops, dev, dtype, (n, 2 * h, 2 * w, c), pg, NAN, dy).snap()
        xb = Buf(ops, dev, dtype, (n, h, w, c), px, 7.0)
        xb.v.as_nhwc().copy_(old.to(dev)) if accumulate else xb.v.as_nhwc().fill_(NAN)   # (the write form must not read dx)
        xb.snap()
        ops.upsample2x_bwd(gb.v, xb.v, accumulate)
        torch.cuda.synchronize()
        gb.check("upsample2x_bwd dy")
        xb.check("upsample2x_bwd dx", written=True)
        outs[form] = xb.nhwc()
    got = outs["sliced"].double().cpu()
    assert torch.isfinite(got).all()
    assert torch.equal(outs["sliced"], outs["flat"])
    want = ref.to(dtype).double()
    if dtype == torch.float32:
        bound = (3 + accumulate + 1) * 2.0 ** -24 * mag
    else:
        bound = _ulp(ref, dtype)
    bad = ((got - want).abs() > bound).sum().item()
    assert bad == 0, f"{bad} elements beyond the bound, worst {((got - want).abs() / bound.clamp_min(1e-300)).max().item():.3g} x"


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
@pytest.mark.parametrize("no,ny,nx", [(85, 7, 5), (12, 9, 4), (370, 3, 6)], ids=["no85", "no12", "no370"])
def test_detect_raw_bwd_is_a_permutation(dev, dtype, no, ny, nx):
    """y3_detect_raw_bwd: ghead[b, y, x, a * no + o] = graw[b, a, y, x, o] bit for bit, rectangular maps, head channels padded up to a multiple of 8 (255 -> 256, 36 -> 40,
    1110 -> 1112), into a contiguous and into a sliced ghead.  The pad channels: DetectUnit.bwd_from (train_engine.py) takes ghead from plan.scratch_like -- uninitialised
    memory -- and feeds it to y3_conv2d_wgrad and to the data-gradient conv, whose K runs over all padded channels against zero filter rows; it relies on the kernel writing
    ZERO into the pad channels (0 * stale NaN would poison dx), so that is asserted."""
    _lib, ops = _ops()
    bs, na = 2, 3
    cpad = (na * no + 7) // 8 * 8
    g = torch.Generator().manual_seed(no)
    graw = torch.randn(bs, na, ny, nx, no, generator=g).to(dtype).to(dev)
    want = graw.permute(0, 2, 3, 1, 4).reshape(bs, ny, nx, na * no)
    vec = 4 if dtype == torch.float32 else 8
    for pads in (None, (2 * vec, 6 * vec)):
        hb = Buf(ops, dev, dtype, (bs, ny, nx, cpad), pads, 7.0)
        hb.v.as_nhwc().fill_(NAN)
        hb.snap()
        ops.detect_raw_bwd(graw, na, no, hb.v)
        torch.cuda.synchronize()
        hb.check("detect_raw_bwd ghead", written=True)
        got = hb.nhwc()
        assert torch.equal(bits(got[..., : na * no].contiguous()), bits(want.contiguous())), "not the permutation of graw"
        assert torch.all(got[..., na * no :] == 0), "pad channels of ghead are not zero"


# ------------------------------------------------------------------------------------------------ descriptor reach by pitch alone
def test_conv_beyond_2gib_by_pitch_alone(dev):
    """test_conv_beyond_2gib_output's sibling: the input's own channels hold 0.2 GB, but it is a 32-channel slice of a 352-channel buffer, so its pitched extent (2.16 GB) passes
    the 2^31-byte reach of a buffer descriptor -- the image-range split of conv_fwd_impl is triggered by the pitch alone.  First, middle (either side of the split) and last
    image against conv2d; the neighbours are NaN."""
    _lib, ops = _ops()
    n, h, w, cin, cout, pitch = 30, 320, 320, 32, 32, 352
    dtype = torch.float16
    need = n * h * w * pitch * 2 + (2 << 30)
    free = torch.cuda.mem_get_info(dev)[0]
    if free < need:
        pytest.skip(f"needs {need / 2**30:.1f} GiB of free device memory, the card has {free / 2**30:.1f}")
    g = torch.Generator().manual_seed(5)
    wt = torch.randn(cout, cin, 1, 1, generator=g) / math.sqrt(cin)
    b = torch.randn(cout, generator=g) * 0.5
    filt = ops.pack_filter(wt.to(dev), cout, cin, dtype)
    xbig, xv = wide_view(ops, n, h, w, cin, dtype, dev, (64, pitch - 64 - cin), NAN)
    assert xv.buf.numel() * 2 > 2**31 and n * h * w * cin * 2 < 2**31
    gd = torch.Generator(device=dev).manual_seed(5)
    for img in range(n):   # (image by image: no second 2 GB temporary)
        xv.as_nhwc()[img] = (torch.rand(h, w, cin, device=dev, generator=gd) * 2 - 1).to(dtype)
    ybig, yv = wide_view(ops, n, h, w, cout, dtype, dev, PY, 7.0)
    ops.conv2d(xv, filt, b.to(dev), yv, 1, 1, True, None, workspace=conv_ws(dev))
    torch.cuda.synchronize()
    full = ybig.as_nhwc()
    assert torch.all(full[..., : PY[0]] == 7.0) and torch.all(full[..., PY[0] + cout :] == 7.0), "conv wrote outside its channel slice"
    assert torch.isnan(xbig.as_nhwc()[0, 0, 0, 0]).item() and torch.isnan(xbig.as_nhwc()[n - 1, h - 1, w - 1, pitch - 1]).item()
    for img in (0, n // 2 - 1, n // 2, n - 1):
        xi = xv.as_nhwc()[img].float().cpu().permute(2, 0, 1)[None]
        ref = F.silu(F.conv2d(xi, wt.to(dtype).float(), b))
        out = yv.as_nhwc()[img].float().cpu().permute(2, 0, 1)[None]
        _conv_tol_check(f"img{img}", dtype, out, ref)
