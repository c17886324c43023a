"""-m gpu: the tiled Detect decode (csrc/detect_nms.hip::decode_tile_kernel, knob decode_tile) and y3_detect_decode_levels.

What is pinned, and against what:
  * the 64 Ki-entry sigmoid table IS the expression of decode_one: every bit pattern of fp16 / bf16 through the tiled kernel (table in LDS, table in global memory, computed
    sigmoid) equals the path before it (decode_tile = 0: decode_vec_kernel / decode_kernel) bit for bit, NaN patterns included;
  * values: the CPU restatement of the reference's Detect (oracle.detect_decode, models/yolo.py:104-108 run in the tensor dtype) by the criterion of
    test_detect_decode_vs_reference_golden, and tests/golden/decode.pt through the Detect module;
  * the three call forms (raw + z, z only into a window, raw only), arguments the tiled kernel does not take (fp32, a pitch or a window off the 16-byte grid, a level whose
    ny * nx * no is no multiple of 8) and the bytes a call must leave alone.

Shapes: a tile is 1024 // ceil(3 * no / 8) pixels rounded down to whole 16-byte groups (32 pixels at no 85, 340 at no 6, 4 at no 370), so 8 x 8 is two full tiles, 4 x 12 a full
and a partial one and 20 x 20 has a partial last tile at no 85; no 6 puts two pixel boundaries into one thread's 8 elements, no 370 none or one.
"""
import pytest
import torch

from oracle import yolo_oracle as yo
from test_gpu_parity import _decode_close, bits

pytestmark = pytest.mark.gpu

NA = 3
ANCHORS = [[10, 13, 16, 30, 33, 23], [30, 61, 62, 45, 59, 119], [116, 90, 156, 198, 373, 326]]
STRIDES = [8.0, 16.0, 32.0]
GRIDS = [(8, 8), (4, 12), (20, 20)]
SENTINEL = 777.0
TILED = (1, 2, 3, 4)   # decode_tile: auto / table in LDS / computed sigmoid / table in global memory


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


def _dt(dtype):
    return str(dtype).split(".")[-1]


def _consts(dtype, nl):
    """(anchors in grid units as the Detect module holds them, per level anchors in pixels / stride as engine._decode_consts hands them to the library)"""
    stride = torch.tensor(STRIDES[:nl]).to(dtype)
    grid_units = (torch.tensor(ANCHORS[:nl]).float().view(nl, NA, 2) / torch.tensor(STRIDES[:nl]).view(-1, 1, 1)).to(dtype)
    apx = (grid_units * stride.view(-1, 1, 1)).float()
    return grid_units, [apx[l].reshape(-1).tolist() for l in range(nl)], [float(s) for s in stride]


_CASES = {}


def _case(dtype, no, grids, bs):
    """(head maps (bs, na * no, ny, nx) per level, expected raw per level, expected z (bs, rows, no)) on the CPU, computed once per case and never modified"""
    key = (dtype, no, tuple(grids), bs)
    if key not in _CASES:
        g = torch.Generator().manual_seed(no * 1000 + len(grids) * 10 + bs)
        xs = [(torch.randn(bs, NA * no, ny, nx, generator=g) * 2.0).to(dtype) for ny, nx in grids]
        raws = [x.view(bs, NA, no, x.shape[2], x.shape[3]).permute(0, 1, 3, 4, 2).contiguous() for x in xs]
        if dtype == torch.float32:
            z = yo.detect_decode(raws, _consts(dtype, len(grids))[0], torch.tensor(STRIDES[: len(grids)]))
        else:
            z = yo.detect_decode(raws, _consts(dtype, len(grids))[0], torch.tensor(STRIDES[: len(grids)]).to(dtype))
        _CASES[key] = (xs, raws, z)
    return _CASES[key]


def _heads(ops, dev, xs, dtype, pitch_of):
    """NHWC head views with pitch_of(channels) elements per pixel, the pad channels holding SENTINEL"""
    hs = []
    for x in xs:
        bs, c, ny, nx = x.shape
        hv = ops.View.alloc(bs, ny, nx, c, dtype, dev, pitch=pitch_of(c))
        hv.buf.fill_(SENTINEL)
        hv.as_nhwc().copy_(x.permute(0, 2, 3, 1).to(dev))
        hs.append(hv)
    return hs


def _pad8(c):
    return (c + 8) // 8 * 8   # 255 -> 256, 18 -> 24, 1110 -> 1112: always at least one pad channel


def _decode(ops, dev, xs, dtype, no, *, levels, want_raw=True, want_z=True, off=0, total=None, pitch_of=_pad8):
    """decode every level of `xs`, by ONE y3_detect_decode_levels call (levels=True; returns None where the library refuses) or level by level.
    -> (False where the levels call refused, raws or None, z buffer (bs, total, no) or None), the outputs pre-filled with SENTINEL"""
    bs = xs[0].shape[0]
    rows = [NA * x.shape[2] * x.shape[3] for x in xs]
    total = sum(rows) + off if total is None else total
    _, apx, strides = _consts(dtype, len(xs))
    hs = _heads(ops, dev, xs, dtype, pitch_of)
    raws = [torch.full((bs, NA, x.shape[2], x.shape[3], no), SENTINEL, dtype=dtype, device=dev) for x in xs] if want_raw else None
    z = torch.full((bs, total, no), SENTINEL, dtype=dtype, device=dev) if want_z else None
    offs = [off + sum(rows[:l]) for l in range(len(xs))]
    if levels:
        ok = ops.detect_decode_levels(hs, NA, no, apx, strides, raws, z, offs, total)
        torch.cuda.synchronize()
        return ok, raws, z
    for l, hv in enumerate(hs):
        ops.detect_decode(hv, NA, no, apx[l], strides[l], raws[l] if want_raw else None, z, offs[l], total)
    torch.cuda.synchronize()
    return True, raws, z


def _same(a, b):
    return torch.equal(bits(a), bits(b))


# ------------------------------------------------------------------------------------------------ 1. the table against the path before it
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=_dt)
def test_every_bit_pattern_equals_the_previous_path(dev, tune, dtype):
    """all 65 536 bit patterns of the dtype as one head (bs 2, 16 x 16 pixels, na 3, no 85: 130 560 elements, pattern = flat index mod 65 536, so every pattern stands at two
    channels): raw and z of the tiled kernel in each of its sigmoid forms are the bits of decode_tile = 0"""
    from yolov3_amd import ops

    bs, ny, nx, no = 2, 16, 16, 85
    pat = torch.arange(bs * NA * no * ny * nx, dtype=torch.int32).remainder(65536)
    pat = torch.where(pat >= 32768, pat - 65536, pat).to(torch.int16)
    assert pat.unique().numel() == 65536
    x = pat.view(dtype).view(bs, ny, nx, NA * no).permute(0, 3, 1, 2).contiguous()   # the patterns run along the channels of a pixel, as they lie in the head
    out = {}
    for knob in (0,) + TILED:
        tune("decode_tile", knob)
        _, raws, z = _decode(ops, dev, [x], dtype, no, levels=False)
        out[knob] = (raws[0].cpu(), z.cpu())
    want_raw = x.view(bs, NA, no, ny, nx).permute(0, 1, 3, 4, 2).contiguous()
    assert _same(out[0][0], want_raw)
    nan = torch.isnan(out[0][1].float()).sum().item()
    print(f"[decode tile patterns] {_dt(dtype)}: {nan} NaN elements of {out[0][1].numel()} in z")
    assert nan > 0
    for knob in TILED:
        assert _same(out[knob][0], out[0][0]), f"raw differs at decode_tile = {knob}"
        assert _same(out[knob][1], out[0][1]), f"z differs at decode_tile = {knob}: {(bits(out[knob][1]) != bits(out[0][1])).sum().item()} elements"


# ------------------------------------------------------------------------------------------------ 2. values
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=_dt)
@pytest.mark.parametrize("no", [85, 6, 370])
def test_values_against_the_cpu_restatement(dev, tune, no, dtype):
    """three levels (8 x 8, 4 x 12, 20 x 20; bs 2; pitch = channels rounded up past one pad channel) by one levels call, level by level, and with decode_tile = 0: all
    bit-equal, raw the permuted head, z within the decode criterion of the oracle's restatement in the same dtype"""
    from yolov3_amd import ops

    xs, want_raws, want_z = _case(dtype, no, GRIDS, 2)
    tune("decode_tile", 0)
    _, raws0, z0 = _decode(ops, dev, xs, dtype, no, levels=False)
    for r, w in zip(raws0, want_raws):
        assert _same(r.cpu(), w), "raw is not the permuted head"
    zc = z0.cpu()
    print(f"[decode tile values] no {no} {_dt(dtype)}: {(zc.float() != want_z.float()).float().mean().item():.2e} of {zc.numel()} elements differ from the restatement, "
          f"max {(zc.float() - want_z.float()).abs().max().item():.3e}")
    _decode_close(zc.float(), want_z.float(), dtype)
    for knob in TILED:
        tune("decode_tile", knob)
        for levels in (True, False):
            ok, raws, z = _decode(ops, dev, xs, dtype, no, levels=levels)
            assert ok, "the library refused eligible levels"
            assert _same(z, z0) and all(_same(a, b) for a, b in zip(raws, raws0)), (knob, levels)


def test_fp32_and_odd_pitch_take_the_element_kernels(dev, tune):
    """fp32 (any pitch) and a 2-byte head whose pitch is its 255 channels (rows off the 16-byte grid) are refused by the levels call and decoded by y3_detect_decode as before"""
    from yolov3_amd import ops

    for dtype, pitch_of in ((torch.float32, _pad8), (torch.float16, lambda c: c)):
        xs, want_raws, want_z = _case(dtype, 85, GRIDS[:2], 2)
        got = {}
        for knob in (0, 1):
            tune("decode_tile", knob)
            _, raws, z = _decode(ops, dev, xs, dtype, 85, levels=False, pitch_of=pitch_of)
            got[knob] = (raws, z)
            for r, w in zip(raws, want_raws):
                assert _same(r.cpu(), w)
            _decode_close(z.cpu().float(), want_z.float(), dtype)
        assert _same(got[0][1], got[1][1])
        ok, raws, z = _decode(ops, dev, xs, dtype, 85, levels=True, pitch_of=pitch_of)
        assert not ok and (z == SENTINEL).all() and all((r == SENTINEL).all() for r in raws), "a refused levels call wrote something"


@pytest.mark.parametrize("key,dtype,nc", [("nc80-float16", torch.float16, 80), ("nc3-float16", torch.float16, 3), ("nc80-float32", torch.float32, 80)])
@pytest.mark.parametrize("knob", [0, 1, 2])
def test_detect_module_against_decode_golden(dev, tune, golden_dir, knob, key, dtype, nc):
    """test_detect_decode_vs_reference_golden (the unmodified reference's output, tests/golden/decode.pt) through the Detect module with the knob at 0, 1 and 2"""
    from yolov3_amd import Detect

    tune("decode_tile", knob)
    gold = torch.load(golden_dir / "decode.pt")[key]
    no = nc + 5
    g = torch.Generator().manual_seed(21)
    xs = [torch.randn(2, 3 * no, s, s + 1, generator=g) * 2.0 for s in gold["sizes"]]
    det = Detect(nc, ANCHORS, ch=(3 * no,) * 3)
    det.stride = torch.tensor(STRIDES)
    det.anchors /= det.stride.view(-1, 1, 1)
    for conv in det.m:  # identity head so the decode sees exactly the seeded maps
        conv.weight.data = torch.eye(3 * no).view(3 * no, 3 * no, 1, 1)
        conv.bias.data.zero_()
    det = det.to(dev).to(dtype).eval()
    z, raw = det([x.to(dev).to(dtype) for x in xs])
    torch.cuda.synchronize()
    for r, x in zip(raw, xs):
        assert torch.equal(r.cpu(), x.to(dtype).view(2, 3, no, x.shape[2], x.shape[3]).permute(0, 1, 3, 4, 2)), "raw (bs,na,ny,nx,no) layout mismatch"
    assert z.dtype == gold["z"].dtype and z.shape == gold["z"].shape
    _decode_close(z.float().cpu(), gold["z"].float(), dtype)


# ------------------------------------------------------------------------------------------------ 3. forms, 6. untouched bytes
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=_dt)
def test_call_forms_and_windows(dev, tune, dtype):
    """raw only (training) and z only into rows [225, 450) of a 1 000-row buffer -- the 96 x 160 tiny-model window of DESIGN (levels of 6 x 10 and 3 x 5, 225 rows) behind
    another member's 225 rows: 225 * 85 elements are off the 16-byte grid (and so are the levels' own blocks), so the element kernels run whatever the knob says.  Then a head
    the tiled kernel takes (8 x 8 and 4 x 12) into rows [224, 464) of such a buffer, and raw only.  The window's rows hold the restatement's values, every other row of the
    buffer keeps its sentinel, and all of it equals decode_tile = 0.  (raw + z: test_values_against_the_cpu_restatement.)"""
    from yolov3_amd import ops

    no, grids = 85, [(6, 10), (3, 5)]
    xs, want_raws, want_z = _case(dtype, no, grids, 2)
    rows = want_z.shape[1]
    assert rows == 225
    ref = None
    for knob in (0, 1, 2):
        tune("decode_tile", knob)
        ok, _, _ = _decode(ops, dev, xs, dtype, no, levels=True)
        assert not ok, "60 * 85 and 15 * 85 elements per (image, anchor) are no multiples of 8: the levels call refuses this head"
        _, raws, z = _decode(ops, dev, xs, dtype, no, levels=False, want_z=False)   # raw only
        assert z is None and all(_same(r.cpu(), w) for r, w in zip(raws, want_raws))
        _, raws, z = _decode(ops, dev, xs, dtype, no, levels=False, want_raw=False, off=225, total=1000)   # z only, into the window
        zc = z.cpu()
        outside = torch.ones(1000, dtype=torch.bool)
        outside[225 : 225 + rows] = False
        assert raws is None and (zc[:, outside] == SENTINEL).all(), "rows outside the window were written"
        _decode_close(zc[:, 225 : 225 + rows].float(), want_z.float(), dtype)
        ref = zc if ref is None else ref
        assert _same(zc, ref), knob
    # an eligible head (8 x 8 and 4 x 12) through the levels call: z only at an aligned window, raw only
    xs, want_raws, want_z = _case(dtype, no, GRIDS[:2], 2)
    rows = want_z.shape[1]
    tune("decode_tile", 0)
    _, _, z0 = _decode(ops, dev, xs, dtype, no, levels=False, want_raw=False, off=224, total=1000)
    _decode_close(z0.cpu()[:, 224 : 224 + rows].float(), want_z.float(), dtype)
    for knob in TILED:
        tune("decode_tile", knob)
        ok, raws, z = _decode(ops, dev, xs, dtype, no, levels=True, want_raw=False, off=224, total=1000)
        assert ok and raws is None, "the library refused eligible levels"
        assert _same(z, z0)
        outside = torch.ones(1000, dtype=torch.bool)
        outside[224 : 224 + rows] = False
        assert (z[:, outside.to(dev)] == SENTINEL).all(), "rows outside the window were written"
        ok, raws, z = _decode(ops, dev, xs, dtype, no, levels=True, want_z=False)
        assert ok and z is None and all(_same(r.cpu(), w) for r, w in zip(raws, want_raws))


def test_pad_channel_never_reaches_raw_and_head_is_not_written(dev, tune):
    """channel 255 of the 256-pitch head holds a sentinel: no element of raw or z carries it, and the head buffer keeps its bits"""
    from yolov3_amd import ops

    dtype, no = torch.float16, 85
    xs, want_raws, _ = _case(dtype, no, GRIDS, 2)
    _, apx, strides = _consts(dtype, 3)
    for knob in (1, 2):
        tune("decode_tile", knob)
        hs = _heads(ops, dev, xs, dtype, _pad8)
        before = [h.buf.clone() for h in hs]
        rows = [NA * x.shape[2] * x.shape[3] for x in xs]
        raws = [torch.zeros(2, NA, x.shape[2], x.shape[3], no, dtype=dtype, device=dev) for x in xs]
        z = torch.zeros(2, sum(rows), no, dtype=dtype, device=dev)
        assert ops.detect_decode_levels(hs, NA, no, apx, strides, raws, z, [0, rows[0], rows[0] + rows[1]], sum(rows))
        torch.cuda.synchronize()
        assert all(_same(h.buf, b) for h, b in zip(hs, before)), "decode wrote into its input"
        assert all((h.as_nhwc().shape[-1] == 255 and (h.buf.view(-1, 256)[:, 255] == SENTINEL).all()) for h in hs)
        assert not any((r == SENTINEL).any() for r in raws) and all(_same(r.cpu(), w) for r, w in zip(raws, want_raws))


# ------------------------------------------------------------------------------------------------ 4. an ineligible level
def test_ineligible_level(dev, tune):
    """5 x 7 pixels: 35 * 85 elements per (image, anchor) is no multiple of 8.  The single-level call falls back with equal values; the levels call on a head that contains
    the level returns non-zero, names the reason and writes nothing."""
    from yolov3_amd import _lib, ops

    dtype, no = torch.float16, 85
    xs, want_raws, want_z = _case(dtype, no, [(8, 8), (5, 7)], 2)
    got = {}
    for knob in (0, 1):
        tune("decode_tile", knob)
        _, raws, z = _decode(ops, dev, xs, dtype, no, levels=False)
        assert all(_same(r.cpu(), w) for r, w in zip(raws, want_raws))
        _decode_close(z.cpu().float(), want_z.float(), dtype)
        got[knob] = z
    assert _same(got[0], got[1])
    ok, raws, z = _decode(ops, dev, xs, dtype, no, levels=True)
    assert not ok
    assert b"cannot take the tiled kernel" in _lib.lib().y3_last_error()
    assert (z == SENTINEL).all() and all((r == SENTINEL).all() for r in raws), "a refused levels call wrote something"


# ------------------------------------------------------------------------------------------------ 5. levels call against single calls, and through the model
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=_dt)
@pytest.mark.parametrize("hw", [64, 128])
def test_levels_call_equals_single_calls(dev, tune, hw, dtype):
    """the three levels of a yolov3 input (bs 2) in one launch == three y3_detect_decode calls with decode_tile = 0.  128 x 128 (16 x 16, 8 x 8, 4 x 4): the levels call takes
    them.  64 x 64 (8 x 8, 4 x 4, 2 x 2): the 2 x 2 level has 4 * 85 = 340 elements per (image, anchor) -- no multiple of 8, the eligibility rule -- so the levels call must
    refuse the head and write nothing, and what a caller then does (engine._decode_outputs: level by level) gives the same bits."""
    from yolov3_amd import ops

    grids = [(hw // 8, hw // 8), (hw // 16, hw // 16), (hw // 32, hw // 32)]
    xs, want_raws, want_z = _case(dtype, 85, grids, 2)
    tune("decode_tile", 0)
    _, raws0, z0 = _decode(ops, dev, xs, dtype, 85, levels=False)
    _decode_close(z0.cpu().float(), want_z.float(), dtype)
    for knob in TILED:
        tune("decode_tile", knob)
        ok, raws, z = _decode(ops, dev, xs, dtype, 85, levels=True)
        assert ok == (hw == 128), "the levels call takes exactly the heads whose every level is eligible"
        if not ok:
            assert (z == SENTINEL).all() and all((r == SENTINEL).all() for r in raws), "a refused levels call wrote something"
            _, raws, z = _decode(ops, dev, xs, dtype, 85, levels=False)
        assert _same(z, z0) and all(_same(a, b) for a, b in zip(raws, raws0)), knob


def test_model_forward_is_unchanged_by_the_knob(dev, tune):
    """model(x) of yolov3 at 64 x 64, bs 2, fp16: prediction and raw maps with decode_tile = 1 and 2 are the bits of decode_tile = 0"""
    from yolov3_amd import DetectionModel

    torch.manual_seed(3)
    m = DetectionModel("yolov3.yaml", nc=80).to(dev).half().eval()
    x = torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(4)).to(dev).half()
    out = {}
    for knob in (0, 1, 2):
        tune("decode_tile", knob)
        pred, raw = m(x)
        torch.cuda.synchronize()
        out[knob] = (pred.clone(), [r.clone() for r in raw])
    assert out[0][0].shape == (2, 3 * (64 + 16 + 4), 85)
    for knob in (1, 2):
        assert _same(out[knob][0], out[0][0]) and all(_same(a, b) for a, b in zip(out[knob][1], out[0][1])), knob


# ------------------------------------------------------------------------------------------------ 7. determinism
def test_two_runs_are_bit_equal(dev, tune):
    from yolov3_amd import ops

    xs, _, _ = _case(torch.float16, 85, GRIDS, 2)
    for knob in (1, 2):
        tune("decode_tile", knob)
        a = _decode(ops, dev, xs, torch.float16, 85, levels=True)
        b = _decode(ops, dev, xs, torch.float16, 85, levels=True)
        assert a[0] and b[0] and _same(a[2], b[2]) and all(_same(p, q) for p, q in zip(a[1], b[1]))
