"""-m gpu: every kernel that walks the prediction rows (.., no = nc + 5) across class counts 1 .. 365 -- the loss kernels (csrc/loss.hip), decode and the NMS candidate
kernel (csrc/detect_nms.hip), and a whole train step with 1 and 2 classes (head convs with 18 / 21 real filters inside a padded pitch) -- against the CPU oracle, which
tests/test_oracle_vs_reference_live.py pins to the unmodified reference at nc 1 / 2 / 3 / 60 (tests/golden/class_counts.pt).

What selects a code path, and the sizes that stand on both sides of it:
  * loss_obj_kernel<T, 1>: 8 (2-byte types) or 4 (fp32) consecutive elements per thread, the objectness positions and the cell cursor worked out from no:
    no 6 / 7 (two objectness elements in one run of 8), 8 / 9, 16, and a level whose cells * no is no multiple of 8 or 4 (the scalar tail);
  * loss_match_kernel / loss_scatter_kernel: lanes stride the class logits / the row 64 at a time: no 64 / 65 / 69 / 70, 128 / 129, 370; nc = 1 drops the class loss;
  * decode_vec_kernel (2-byte types, no >= 8, 16-byte aligned blocks) against decode_kernel: no 6 .. 65;
  * nms_candidates_kernel: nc <= 64, <= 128, above; multi_label only with nc > 1.
"""
from pathlib import Path

import pytest
import torch
import yaml

import class_count_cases as cc
from oracle import yolo_oracle as yo
from test_gpu_parity import _cmp_nms, _decode_close, bits, build_pair, checksum, wide_view

pytestmark = pytest.mark.gpu

CFG = Path(__file__).resolve().parents[1] / "yolov3_amd" / "cfg"
STRIDES = {"yolov3": (8, 16, 32), "yolov3-tiny": (16, 32)}
NAN = float("nan")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


def _dt(dtype):
    return str(dtype).split(".")[-1]


# ------------------------------------------------------------------------------------------------ loss
class _HeadOnly(torch.nn.Module):
    """what ComputeLoss reads of a model: `hyp` and the Detect module at model[-1] (na, nc, nl, anchors in grid units, stride) -- without the backbone, which a loss test
    on synthetic raw predictions never runs"""

    def __init__(self, name, nc, hyp):
        super().__init__()
        from yolov3_amd import Detect

        det = Detect(nc, yaml.safe_load(open(CFG / f"{name}.yaml"))["anchors"], ch=(8,) * len(STRIDES[name]))
        det.stride = torch.tensor([float(s) for s in STRIDES[name]])
        det.anchors /= det.stride.view(-1, 1, 1)
        self.model = torch.nn.ModuleList([det])
        self.hyp = hyp


_LOSS_REF = {}


def _loss_reference(name, nc, hw, bs, dtype, dup):
    """(targets, raw predictions, oracle loss / items / gradients of 1024 * loss) of one case, computed once: the oracle on the dtype-rounded inputs in fp32"""
    key = (name, nc, hw, bs, dtype, dup)
    if key not in _LOSS_REF:
        anchors = torch.tensor(yaml.safe_load(open(CFG / f"{name}.yaml"))["anchors"]).float().view(len(STRIDES[name]), -1, 2)
        anchors = anchors / torch.tensor([float(s) for s in STRIDES[name]]).view(-1, 1, 1)
        shapes = [(bs, 3, hw // s, hw // s, nc + 5) for s in STRIDES[name]]
        _, tg = cc.pick_targets(bs, nc, shapes, anchors, 300 + nc)
        if dup:   # the stack of test_loss_backward_is_bit_deterministic_on_duplicated_cells: every cell matched three times, by boxes of different size, rows shuffled
            tg = torch.cat((tg, tg * torch.tensor([1, 1, 1, 1, 0.9, 1.1]), tg * torch.tensor([1, 1, 1, 1, 1.15, 0.85])))
            tg[:, 1] = tg[:, 1].round().clamp(0, nc - 1)
            tg = tg[torch.randperm(tg.shape[0], generator=torch.Generator().manual_seed(1))]
        classes = set(tg[:, 1].long().tolist())
        assert nc - 1 in classes and (nc > 4 or classes == set(range(nc))), f"nc {nc}: the targets name the classes {sorted(classes)}"
        p_cpu = yo.synth_raw_predictions(shapes, seed=400 + nc)
        p_ref = [t.to(dtype).float().clone().requires_grad_(True) for t in p_cpu]
        loss, items, _ = yo.compute_loss(p_ref, tg, anchors, cc.HYP, nc)
        (loss * 1024.0).sum().backward()
        _LOSS_REF[key] = (tg, p_cpu, loss.detach(), items, [t.grad for t in p_ref])
    return _LOSS_REF[key]


# gradient bound: max |device - oracle| over a level, relative to the level's largest oracle gradient.  fp16 2e-3 is the bound of test_loss_vs_oracle_variants[fp16].
# bf16 keeps 3 mantissa bits fewer than fp16: 8 x the fp16 bound, on the loss (rtol / atol) and on the gradients alike.
# Measured on an MI355X (worst case per head; the bounds are NOT derived from these; also in DESIGN.md, parity section): bf16 3.37e-3 on the three-level head (nc 123),
# 3.40e-3 on the two-level head (nc 2), 3.08e-3 on the scalar-tail case, 3.11e-3 with duplicated cells; fp16 4.8e-4 / 4.3e-4 / 3.9e-4 / 4.8e-4; fp32 2.8e-7.  The
# figure hardly moves with nc: it is the objectness plane's (tobj is rounded to T on the device, kept in fp32 by the oracle).
HALF_GRAD_BOUND = {torch.float16: 2e-3, torch.bfloat16: 1.6e-2}


def _check_loss_case(dev, name, nc, hw, bs, dtype, dup=False):
    from yolov3_amd import ComputeLoss

    no = nc + 5
    tg, p_cpu, ref_loss, ref_items, ref_grads = _loss_reference(name, nc, hw, bs, dtype, dup)
    crit = ComputeLoss(_HeadOnly(name, nc, dict(cc.HYP)).to(dev))
    p = [t.to(dev).to(dtype).requires_grad_(True) for t in p_cpu]
    runs = []
    for _ in range(2):
        for t in p:
            t.grad = None
        loss, items = crit(p, tg.to(dev))
        (loss * 1024.0).sum().backward()   # (a GradScaler-style upstream gradient)
        torch.cuda.synchronize()
        runs.append([t.grad.clone() for t in p])
    loss, items = loss.detach().cpu(), items.cpu()
    what = f"[class counts loss] {name} nc {nc} no {no} {hw} px bs {bs} {_dt(dtype)}{' dup' if dup else ''}"
    half = HALF_GRAD_BOUND.get(dtype)
    tol = dict(rtol=1e-4, atol=1e-5) if half is None else dict(rtol=half, atol=half)
    worst = 0.0
    for lvl, (g_dev, want) in enumerate(zip(runs[0], ref_grads)):
        assert g_dev.dtype == dtype and g_dev.shape == want.shape
        g = g_dev.float().cpu()
        worst = max(worst, (g - want).abs().max().item() / want.abs().max().item())
    print(f"{what}: loss {loss.item():.6f} (oracle {ref_loss.item():.6f}), worst gradient error relative to the level's max {worst:.3e}")
    torch.testing.assert_close(loss, ref_loss, **tol)
    torch.testing.assert_close(items, ref_items, **tol)
    for lvl, (g_dev, want) in enumerate(zip(runs[0], ref_grads)):
        g = g_dev.float().cpu()
        # the set of non-zero elements outside channel 4: a row written to the wrong cell or channel shows here even when its values are small against the level's max.
        # A device zero is allowed where the oracle's value is below the dtype's smallest normal number.
        tiny = torch.finfo(dtype).tiny
        bad = ((g != 0) != (want != 0)) & ~((g == 0) & (want.abs() < tiny))
        bad[..., 4] = False
        if bad.any():
            first = int(bad.reshape(-1).nonzero()[0])
            raise AssertionError(f"{what}: level {lvl}: {int(bad.sum())} elements are zero on one side only; first at flat index {first} (cell {first // no}, channel {first % no}): "
                                 f"device {g.reshape(-1)[first].item()}, oracle {want.reshape(-1)[first].item()}")
        err = (g - want).abs()
        if half is None:
            ok = err <= 1e-6 * 1024.0 + 1e-4 * want.abs()   # (assert_close(rtol=1e-4, atol=1e-6 * scale), with the place of the first miss)
        else:
            ok = err < half * want.abs().max()
        if not ok.all():
            first = int((~ok).reshape(-1).nonzero()[0])
            raise AssertionError(f"{what}: level {lvl}: {int((~ok).sum())} gradient elements out of bound, worst {err.max().item():.3e} against a level max of {want.abs().max().item():.3e}; "
                                 f"first at flat index {first} (cell {first // no}, channel {first % no}): device {g.reshape(-1)[first].item()}, oracle {want.reshape(-1)[first].item()}")
        if nc == 1:
            assert not g_dev[..., 5].any(), f"{what}: level {lvl}: the only class logit has a gradient"
    if nc == 1:   # one class: no class loss (reference utils/loss.py:164)
        assert items[2].item() == 0.0
        torch.testing.assert_close(loss, (items[0] + items[1]).reshape(1) * bs, rtol=1e-6, atol=1e-7)   # (fp32 sums of the same kernel: a few ulp)
    for lvl, (a, b) in enumerate(zip(*runs)):
        assert torch.equal(bits(a), bits(b)), f"{what}: level {lvl}: two backward passes differ"


LOSS_NC = [1, 2, 3, 4, 11, 59, 60, 64, 65, 123, 124, 365]
DTYPES = [torch.float32, torch.float16, torch.bfloat16]


@pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
@pytest.mark.parametrize("nc", LOSS_NC)
def test_loss_class_count_sweep_yolov3_head(dev, nc, dtype):
    """ComputeLoss forward + backward on a three-level head at 64 px, bs 2 (8 x 8, 4 x 4 and 2 x 2 cells): no = 6 .. 370."""
    assert [n + 5 for n in LOSS_NC] == [6, 7, 8, 9, 16, 64, 65, 69, 70, 128, 129, 370]
    _check_loss_case(dev, "yolov3", nc, 64, 2, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
@pytest.mark.parametrize("nc", [1, 2, 60])
def test_loss_class_count_sweep_tiny_head(dev, nc, dtype):
    """the two-level head (balance [4, 1] of the five-entry default) at 96 px, bs 3: 6 x 6 and 3 x 3 cells, 3 * 27 * no elements on the last level"""
    _check_loss_case(dev, "yolov3-tiny", nc, 96, 3, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
def test_loss_objectness_writer_scalar_tail(dev, dtype):
    """bs 1 at 96 px with 2 classes: the last level has 27 cells * 7 = 189 elements, no multiple of the 8 / 4 elements a thread of loss_obj_kernel<T, 1> stores at once --
    the last thread of the level writes a run of 5 (2-byte types) or 1 (fp32) through the element loop"""
    assert (1 * 3 * 3 * 3 * 7) % 8 == 5 and (1 * 3 * 3 * 3 * 7) % 4 == 1
    _check_loss_case(dev, "yolov3", 2, 96, 1, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
@pytest.mark.parametrize("nc", [1, 2, 60])
def test_loss_class_count_sweep_duplicated_cells(dev, nc, dtype):
    """targets stacked three deep on the same cells: the winner slot of loss_scatter_kernel sums the rows of all slots of its cell, 64 channels at a time -- no = 6 and 7
    (one partly filled pass) and 65 (one lane into a second pass)"""
    _check_loss_case(dev, "yolov3", nc, 64, 2, dtype, dup=True)


# ------------------------------------------------------------------------------------------------ decode
DECODE_NO = [6, 7, 8, 9, 16, 64, 65]
DECODE_GRIDS = {"8x8": (8, 8, 4), "5x3": (5, 3, 16)}   # ny, nx, bs (so that each case holds a few thousand elements: the criterion bounds a FRACTION of rounding flips)


def _decode_takes_vec(dtype, no, ny, nx, row_offset, total_rows, aligned):
    """the dispatcher's rule (y3_detect_decode): 2-byte type, no >= 8, whole 16-byte groups in every (image, anchor) block of both outputs"""
    return dtype != torch.float32 and no >= 8 and (ny * nx * no) % 8 == 0 and (total_rows * no) % 8 == 0 and (row_offset * no) % 8 == 0 and aligned


def test_decode_sweep_covers_both_kernels():
    """which kernel each case of test_decode_class_count_sweep takes.  no = 6 and 7 never take decode_vec_kernel (its chunk of 8 may cross a pixel boundary only once: no >= 8);
    a multiple of 8 always fills whole 16-byte groups, so no = 8 / 16 / 64 reach decode_kernel in a 2-byte type only through outputs that are not 16-byte aligned."""
    table = {}
    for no in DECODE_NO:
        for grid, (ny, nx, _) in DECODE_GRIDS.items():
            for aligned in (True, False):
                table[no, grid, aligned] = _decode_takes_vec(torch.float16, no, ny, nx, 8, _decode_rows(ny, nx)[1], aligned)
    assert {k for k, v in table.items() if v} == {(no, g, True) for no in (8, 16, 64) for g in DECODE_GRIDS} | {(9, "8x8", True), (65, "8x8", True)}
    for no in DECODE_NO:
        forms = {table[no, grid, aligned] for grid, aligned in DECODE_CASES[no]}
        assert forms == ({False} if no < 8 else {True, False}), (no, forms)
        assert not any(_decode_takes_vec(torch.float32, no, ny, nx, 8, _decode_rows(ny, nx)[1], True) for ny, nx, _ in DECODE_GRIDS.values())


def _decode_rows(ny, nx):
    """(rows of the level, rows of the whole z): 8 rows of other levels in front, then the level, then a tail to a multiple of 8"""
    rows = 3 * ny * nx
    return rows, (8 + rows + 8 + 7) // 8 * 8


# (grid, 16-byte aligned outputs) per no: both grids, and for the multiples of 8 one more with raw and z one element off the 16-byte grid
DECODE_CASES = {no: [("8x8", True), ("5x3", True)] + ([("5x3", False)] if no % 8 == 0 else []) for no in DECODE_NO}


@pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
@pytest.mark.parametrize("no,grid,aligned", [(no, g, al) for no in DECODE_NO for g, al in DECODE_CASES[no]])
def test_decode_class_count_sweep(dev, no, grid, aligned, dtype):
    """ops.detect_decode of one level whose head is a channel slice of a wider NaN-filled NHWC buffer, into rows [8, 8 + na * ny * nx) of a NaN-filled z: `raw` is the
    permuted head bit for bit, the level's rows of z meet the criterion of test_detect_decode_vs_reference_golden against oracle.detect_decode in the same dtype, and
    every other row of z and every channel of the buffer outside the slice keep their bits."""
    from yolov3_amd import ops

    ny, nx, bs = DECODE_GRIDS[grid]
    na, stride, off = 3, 16.0, 8
    rows, total = _decode_rows(ny, nx)
    x = (torch.randn(bs, na * no, ny, nx, generator=torch.Generator().manual_seed(no * 100 + ny)) * 2.0).to(dtype)
    esz = x.element_size()
    c = na * no
    left = 16 // esz * 2
    right = (-(left + c)) % 8 + 8
    big, hv = wide_view(ops, bs, ny, nx, c, dtype, dev, (left, right), NAN)
    hv.as_nhwc().copy_(x.permute(0, 2, 3, 1).to(dev))
    before = big.buf.clone()
    shift = 0 if aligned else 1   # outputs one element off the 16-byte grid: the dispatcher must fall back to the element kernel
    raw_buf = torch.full((bs * rows * no + 8,), NAN, dtype=dtype, device=dev)
    z_buf = torch.full((bs * total * no + 8,), NAN, dtype=dtype, device=dev)
    raw = raw_buf[shift : shift + bs * rows * no].view(bs, na, ny, nx, no)
    z = z_buf[shift : shift + bs * total * no].view(bs, total, no)
    assert (raw.data_ptr() % 16 == 0) == aligned and (z.data_ptr() % 16 == 0) == aligned
    anchors_grid = (torch.tensor([[30.0, 61.0], [62.0, 45.0], [59.0, 119.0]]) / stride).to(dtype)
    apx = (anchors_grid * torch.tensor(stride).to(dtype)).float().reshape(-1).tolist()   # (engine._decode_consts)
    ops.detect_decode(hv, na, no, apx, stride, raw, z, off, total)
    torch.cuda.synchronize()
    want_raw = x.view(bs, na, no, ny, nx).permute(0, 1, 3, 4, 2).contiguous()
    assert torch.equal(bits(raw.cpu()), bits(want_raw)), "raw is not the permuted head"
    assert torch.equal(bits(big.buf), bits(before)), "decode wrote into its input buffer"
    for buf, n in ((raw_buf, bs * rows * no), (z_buf, bs * total * no)):
        edge = torch.cat((buf[:shift], buf[shift + n :]))
        assert torch.isnan(edge).all(), "decode wrote outside its output"
    zc = z.cpu()
    outside = torch.ones(total, dtype=torch.bool)
    outside[off : off + rows] = False
    assert torch.isnan(zc[:, outside]).all(), "rows of z outside the level were written"
    want = yo.detect_decode([want_raw], anchors_grid.view(1, na, 2), torch.tensor([stride]).to(dtype))
    assert want.dtype == dtype and want.shape == (bs, rows, no)
    got = zc[:, off : off + rows].float()
    print(f"[class counts decode] no {no} {grid} {_dt(dtype)} aligned {aligned}: vec {_decode_takes_vec(dtype, no, ny, nx, off, total, aligned)}, "
          f"{(got != want.float()).float().mean().item():.2e} of {got.numel()} elements differ, max {(got - want.float()).abs().max().item():.3e}")
    _decode_close(got, want.float(), dtype)


@pytest.mark.parametrize("nc,dtype", [(1, torch.float32), (1, torch.float16), (2, torch.float32), (2, torch.float16)])
def test_detect_decode_vs_reference_golden_one_and_two_classes(dev, golden_dir, nc, dtype):
    """Detect (eval) with yolov3-tiny's two levels and no = 6 / 7 against the UNMODIFIED reference's output (tests/golden/class_counts.pt), by the criterion of
    test_detect_decode_vs_reference_golden"""
    from yolov3_amd import Detect

    gold = torch.load(golden_dir / "class_counts.pt")["decode"][f"nc{nc}-{_dt(dtype)}"]
    no = nc + 5
    g = torch.Generator().manual_seed(gold["seed"])
    xs = [torch.randn(2, 3 * no, s, s + 1, generator=g) * 2.0 for s in gold["sizes"]]
    assert sum(checksum(x.to(dtype)) for x in xs) == gold["in_sum"]
    det = Detect(nc, gold["anchors"], ch=(3 * no,) * 2)
    det.stride = torch.tensor(gold["strides"])
    det.anchors /= det.stride.view(-1, 1, 1)
    for conv in det.m:  # identity head so the decode sees exactly the seeded maps
        conv.weight.data = torch.eye(3 * no).view(3 * no, 3 * no, 1, 1)
        conv.bias.data.zero_()
    det = det.to(dev).to(dtype).eval()
    z, raw = det([x.to(dev).to(dtype) for x in xs])
    torch.cuda.synchronize()
    zc, ref = z.float().cpu(), gold["z"].float()
    assert z.dtype == gold["z"].dtype and zc.shape == ref.shape
    for r, x in zip(raw, xs):
        exp = x.to(dtype).view(2, 3, no, x.shape[2], x.shape[3]).permute(0, 1, 3, 4, 2)
        assert torch.equal(r.cpu(), exp), "raw (bs,na,ny,nx,no) layout mismatch"
    print(f"[class counts decode golden] nc {nc} {_dt(dtype)}: {(zc != ref).float().mean().item():.2e} of {zc.numel()} elements differ")
    _decode_close(zc, ref, dtype)


# ------------------------------------------------------------------------------------------------ NMS
NMS_NC = [1, 2, 63, 64, 65, 128, 129]
NMS_AGNOSTIC_NC = (64, 129)
_NMS_PRED = {}


def _nms_pred(nc):
    """2 images x 1500 rows, 30 % of them jittered copies of 60 ground-truth boxes.  With conf_thres 0.05 (checked on the CPU with the oracle): 424 .. 486 rows per image
    pass with their best class, 428 .. 2163 (row, class) pairs with multi_label, and every image keeps more than max_det = 50 boxes (122 .. 300 with max_det = 300)."""
    if nc not in _NMS_PRED:
        _NMS_PRED[nc] = yo.synth_predictions(bs=2, n_rows=1500, nc=nc, seed=200 + nc, hits=0.3, n_gt=60)
    return _NMS_PRED[nc]


def _nms_candidates(pred, thr, multi_label):
    """candidates per image: (row, class) pairs with multi_label (only with nc > 1), rows whose best class passes otherwise (reference utils/general.py:702-714)"""
    multi_label = multi_label and pred.shape[2] - 5 > 1
    out = []
    for x in pred:
        x = x[x[:, 4] > thr]
        conf = x[:, 5:] * x[:, 4:5]
        out.append(int((conf > thr).sum()) if multi_label else int((conf.max(1)[0] > thr).sum()))
    return out


@pytest.mark.parametrize("multi_label", [True, False], ids=["multi_label", "best_class"])
@pytest.mark.parametrize("nc,agnostic", [(nc, False) for nc in NMS_NC] + [(nc, True) for nc in NMS_AGNOSTIC_NC],
                         ids=[f"nc{nc}" for nc in NMS_NC] + [f"nc{nc}_agnostic" for nc in NMS_AGNOSTIC_NC])
def test_nms_class_count_sweep(dev, nc, agnostic, multi_label):
    """non_max_suppression against the oracle on both sides of the candidate kernel's regimes (nc <= 64: one ballot per row; <= 128: two; above: the one-row loop), what
    test_nms_vs_oracle_full_size asserts: the same rows in the same order, bit for bit.  Once cut at max_det = 50, once at 300 (the cut inside and outside the result)."""
    from yolov3_amd import non_max_suppression

    pred = _nms_pred(nc)
    cand = _nms_candidates(pred, 0.05, multi_label)
    assert min(cand) >= 300, f"too few candidates for a test of the candidate kernel: {cand}"
    kept = []
    for max_det in (50, 300):
        kw = dict(conf_thres=0.05, iou_thres=0.6, multi_label=multi_label, agnostic=agnostic, max_det=max_det)
        ref = yo.non_max_suppression(pred, **kw)
        kept.append([int(r.shape[0]) for r in ref])
        res = non_max_suppression(pred.to(dev), **kw)
        _cmp_nms(res, ref, str(kw))
    print(f"[class counts nms] nc {nc} multi_label {multi_label} agnostic {agnostic}: candidates {cand}, kept {kept[0]} of max_det 50, {kept[1]} of 300")
    assert max(kept[0]) == 50 and max(kept[1]) > 50, f"no image reaches max_det: {kept}"


def test_nms_one_class_ignores_multi_label(dev):
    """`multi_label &= nc > 1` (reference utils/general.py:673): with one class both settings give the same rows"""
    from yolov3_amd import non_max_suppression

    pred = _nms_pred(1).to(dev)
    a = non_max_suppression(pred, 0.05, 0.6, multi_label=True, max_det=50)
    b = non_max_suppression(pred, 0.05, 0.6, multi_label=False, max_det=50)
    assert len(a) == len(b) == 2
    for x, y in zip(a, b):
        assert x.shape == y.shape and x.shape[0] == 50 and torch.equal(x, y)


# ------------------------------------------------------------------------------------------------ whole model
def _train_inputs(name, nc, hw, bs, sd):
    anchors = sd[[k for k in sd if k.endswith("anchors")][0]]
    shapes = [(bs, 3, hw // s, hw // s, nc + 5) for s in STRIDES[name]]
    _, tg = cc.pick_targets(bs, nc, shapes, anchors, 500 + nc)
    x = torch.rand(bs, 3, hw, hw, generator=torch.Generator().manual_seed(8))
    return x, tg, anchors


def _oracle_step(layers, save, sd, strides, x, tg, anchors, hyp, nc):
    sdg = {k: (v.clone().requires_grad_(True) if v.is_floating_point() and "running" not in k else v.clone()) for k, v in sd.items()}
    raws = yo.forward(layers, save, sdg, x, strides, training=True)
    loss, _, _ = yo.compute_loss(raws, tg, anchors, hyp, nc)
    loss.backward()
    return loss.detach(), sdg


@pytest.mark.parametrize("name,nc", [("yolov3-tiny", 1), ("yolov3-tiny", 2), ("yolov3", 1)])
def test_model_and_train_step_one_and_two_classes(dev, name, nc):
    """64 px, bs 2, fp32.  Eval forward against the oracle within 1e-4 (as test_model_fp32_vs_reference_golden); train-mode forward + ComputeLoss + backward against
    torch autograd over the oracle, every parameter gradient within 2e-3 of the tensor's gradient scale (as test_train_step_gradients_vs_oracle_autograd).  The head
    convs have 3 * (nc + 5) = 18 / 21 filters: the real output channels inside the padded pitch of the head buffer, in the filter gradient, the raw-gradient
    transpose (detect_raw_bwd) and the data gradient from a mostly-padding gradient tensor."""
    from yolov3_amd import ComputeLoss

    hw, bs = 64, 2
    hyp = dict(cc.HYP)
    m, (layers, save, sd, strides) = build_pair(name, nc, 17, dev, torch.float32)
    assert [int(s) for s in strides] == list(STRIDES[name])
    x, tg, anchors = _train_inputs(name, nc, hw, bs, sd)
    torch.testing.assert_close(m.model[-1].anchors.cpu(), anchors)
    with torch.no_grad():
        ref_pred, ref_raw = yo.forward(layers, save, sd, x, strides, training=False)
    pred, raw = m(x.to(dev))
    torch.cuda.synchronize()
    assert pred.shape == ref_pred.shape and pred.shape[2] == nc + 5
    for a, b in zip(raw, ref_raw):
        err = (a.cpu() - b).abs().max().item()
        assert a.shape == b.shape and err < 1e-4, f"{name} nc {nc}: raw logits max abs err {err:.3g}"
    torch.testing.assert_close(pred.cpu(), ref_pred, rtol=1e-4, atol=1e-4)

    loss_ref, sdg = _oracle_step(layers, save, sd, strides, x, tg, anchors, hyp, nc)
    m.train()
    m.hyp = hyp
    crit = ComputeLoss(m)
    loss, items = crit(m(x.to(dev)), tg.to(dev))
    loss.backward()
    torch.cuda.synchronize()
    torch.testing.assert_close(loss.detach().cpu(), loss_ref, rtol=1e-4, atol=1e-5)
    if nc == 1:
        assert items[2].item() == 0.0
    for conv in m.model[-1].m:
        assert conv.weight.grad.shape == (3 * (nc + 5), conv.in_channels, 1, 1) and conv.bias.grad.shape == (3 * (nc + 5),)
    worst = []
    for k, p in m.named_parameters():
        ref = sdg[k].grad
        assert p.grad is not None, f"{k}: no gradient"
        g = p.grad.cpu()
        rel = (g - ref).abs().max().item() / (ref.abs().max().item() + 1e-12)
        worst.append((rel, k))
    worst.sort(reverse=True)
    print(f"[class counts train] {name} nc {nc}: loss {loss.item():.6f} (oracle {loss_ref.item():.6f}), worst gradient mismatches {worst[:3]}")
    assert worst[0][0] < 2e-3, f"worst gradient mismatches: {worst[:5]}"


def test_train_step_autocast_fp16_one_class(dev):
    """one autocast(fp16) step of yolov3-tiny with a single class, 64 px, bs 2: the bounds of test_train_step_autocast_fp16 -- loss within 0.002 of the fp32 oracle's,
    finite gradients, gradient cosine above 0.985 on every tensor of 4096 elements or more"""
    from yolov3_amd import ComputeLoss

    name, nc, hw, bs = "yolov3-tiny", 1, 64, 2
    hyp = dict(cc.HYP)
    m, (layers, save, sd, strides) = build_pair(name, nc, 19, dev, torch.float32)
    x, tg, anchors = _train_inputs(name, nc, hw, bs, sd)
    loss_ref, sdg = _oracle_step(layers, save, sd, strides, x, tg, anchors, hyp, nc)
    m.train()
    m.hyp = hyp
    crit = ComputeLoss(m)
    with torch.autocast("cuda", dtype=torch.float16):
        raws = m(x.to(dev))
        loss, items = crit(raws, tg.to(dev))
    assert raws[0].dtype == torch.float16 and raws[0].shape[-1] == 6
    (loss * 128.0).backward()
    torch.cuda.synchronize()
    rel = abs(loss.item() - loss_ref.item()) / loss_ref.item()
    cos_min, worst = 1.0, None
    for k, p_ in m.named_parameters():
        ref = sdg[k].grad
        if ref is None or ref.numel() < 4096:
            continue
        c = torch.nn.functional.cosine_similarity((p_.grad.float().cpu() / 128.0).flatten(), ref.flatten(), dim=0).item()
        if c < cos_min:
            cos_min, worst = c, k
    print(f"[class counts autocast] {name} nc {nc} fp16: loss rel err {rel:.4f}, min gradient cosine {cos_min:.4f} at {worst}")
    assert rel < 0.002
    assert items[2].item() == 0.0
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in m.parameters())
    assert cos_min > 0.985, f"gradient direction: cosine {cos_min:.4f} at {worst}"
