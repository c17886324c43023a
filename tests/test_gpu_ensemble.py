"""GPU tests of model ensembles and of the row windows behind them: several producers (Ensemble members, TTA passes, the a-priori label rows of --save-hybrid)
writing into windows of one prediction tensor, and `run_batches` with augment / save_hybrid / compute_loss."""
from pathlib import Path

import numpy as np
import pytest
import torch
import yaml

from oracle import yolo_oracle as yo

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
CFG = ROOT / "yolov3_amd" / "cfg"
HYP = dict(box=0.05, cls=0.5, cls_pw=1.0, obj=1.0, obj_pw=1.0, anchor_t=4.0, fl_gamma=0.0, label_smoothing=0.0)
# tests/test_gpu_parity.py::HALF_BOUNDS, float16 (derived there): the half-precision engine against an fp32 reference with the same weights
HALF_F16 = dict(rms=0.001, mx=0.003, corr=0.99999)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


def build_model(name, nc, seed, dev, dtype):
    """a seeded model as tests/test_gpu_parity.py::build_pair builds it"""
    from yolov3_amd import DetectionModel

    d = yaml.safe_load(open(CFG / f"{name}.yaml"))
    layers, save, anchors, nc_v = yo.parse_cfg(d, 3, nc)
    strides = yo.model_strides(layers)
    sd = yo.seeded_state_dict(layers, nc_v, anchors, strides, seed=seed)
    m = DetectionModel(f"{name}.yaml", nc=nc)
    m.load_state_dict(sd)
    return m.to(dev).to(dtype).eval()


def shift_biases(models, seed=3):
    """random heads detect nothing (max confidence 2e-4): objectness + 5, classes + 3 + 2 randn on every Detect bias"""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in models:
            det = m.model[-1]
            for conv in det.m:
                b = conv.bias.detach().float().cpu().view(det.na, -1).clone()
                b[:, 4] += 5.0
                b[:, 5:] += 3.0 + 2.0 * torch.randn(det.na, det.nc, generator=g)
                conv.bias.copy_(b.view(-1).to(conv.bias))


def rel_errors(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    rms = ((a - b).pow(2).mean().sqrt() / b.pow(2).mean().sqrt()).item()
    mx = ((a - b).abs().max() / b.abs().max()).item()
    corr = torch.corrcoef(torch.stack((a, b)))[0, 1].item()
    return rms, mx, corr


def canon(t):
    """rows ordered by (-score, box, class): exact score ties (label rows all have confidence 1) have no order in the reference"""
    t = t.float().cpu()
    keys = torch.stack((-t[:, 4], t[:, 0], t[:, 1], t[:, 2], t[:, 3], t[:, 5]), 1).tolist()
    return t[sorted(range(len(keys)), key=lambda i: keys[i])]


_PAIRS = {}


def pair(dev, dtype):
    """yolov3-tiny and yolov3, nc 80: members whose predictions have different row counts"""
    if dtype not in _PAIRS:
        _PAIRS[dtype] = (build_model("yolov3-tiny", 80, 41, dev, dtype), build_model("yolov3", 80, 42, dev, dtype))
    return _PAIRS[dtype]


# ------------------------------------------------------------------------------------------------ 1: the windows are exact
@pytest.mark.parametrize("bs,h,w", [(2, 64, 64), (3, 96, 160)])
@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["fp16", "fp32"])
def test_ensemble_equals_the_concatenated_members_bit_for_bit(dev, dtype, bs, h, w):
    """Ensemble(x)[0] == cat of every member's own model(x)[0], plain and augmented; through the private out= path with guard rows in front of and behind the
    window, the guard rows keep their sentinel.  (At 96 x 160 the second member's window starts at row 225 and at 64 x 64 at row 60: with no = 85 in fp16 the
    first is 2-byte aligned only, and the levels inside a member at odd offsets as well -- the decode falls back to element stores there.)"""
    from yolov3_amd import Ensemble, engine

    ens = Ensemble(pair(dev, dtype))
    x = torch.rand(bs, 3, h, w, generator=torch.Generator().manual_seed(5)).to(dev).to(dtype)
    for augment in (False, True):
        want = torch.cat([m(x, augment=augment)[0] for m in ens], 1)
        rows = [engine.pred_rows(m, h, w, augment) for m in ens]
        assert rows[0] != rows[1] and want.shape == (bs, sum(rows), 85)
        y, none = ens(x, augment=augment)
        assert none is None and y.dtype == dtype and torch.equal(y, want), (augment, (y != want).sum().item())
        front, back, sentinel = 7, 5, -7.0
        buf = torch.full((bs, front + sum(rows) + back, 85), sentinel, dtype=dtype, device=dev)
        assert ens._predict_into(x, (buf, front), augment) == sum(rows)
        assert torch.equal(buf[:, front:front + sum(rows)], want)
        assert (buf[:, :front] == sentinel).all() and (buf[:, front + sum(rows):] == sentinel).all()


def test_out_window_is_validated_before_anything_runs(dev):
    from yolov3_amd import Ensemble, engine

    tiny, big = pair(dev, torch.float16)
    x = torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(5)).to(dev).half()
    rows = engine.pred_rows(tiny, 64, 64)
    ok = torch.zeros(2, rows + 3, 85, dtype=torch.float16, device=dev)
    assert engine.run_model(tiny, x, out=(ok, 3)) == rows and (ok[:, :3] == 0).all() and torch.equal(ok[:, 3:], tiny(x)[0])
    bad = {
        "dtype": (torch.zeros(2, rows, 85, dtype=torch.float32, device=dev), 0),
        "device": (torch.zeros(2, rows, 85, dtype=torch.float16), 0),
        "no": (torch.zeros(2, rows, 84, dtype=torch.float16, device=dev), 0),
        "batch": (torch.zeros(3, rows, 85, dtype=torch.float16, device=dev), 0),
        "fit": (torch.zeros(2, rows + 3, 85, dtype=torch.float16, device=dev), 4),
        "negative": (torch.zeros(2, rows + 3, 85, dtype=torch.float16, device=dev), -1),
        "contiguous": (torch.zeros(2, rows, 170, dtype=torch.float16, device=dev)[:, :, :85], 0),
    }
    for what, out in bad.items():
        with pytest.raises(ValueError):
            engine.run_model(tiny, x, out=out)
        assert not out[0].any(), what
    with pytest.raises(ValueError):   # the second member does not fit: the first must not have run either
        buf = torch.zeros(2, rows + 10, 85, dtype=torch.float16, device=dev)
        Ensemble([tiny, big])._predict_into(x, (buf, 0))
    assert not buf.any()
    with pytest.raises(TypeError, match="dtype"):
        Ensemble([tiny, pair(dev, torch.float32)[1]])(x)
    with pytest.raises(ValueError, match="row width"):
        Ensemble([tiny, build_model("yolov3-tiny", 3, 1, dev, torch.float16)])(x)
    with pytest.raises(NotImplementedError):
        Ensemble([tiny, big])(x, visualize=True)


# ------------------------------------------------------------------------------------------------ 2: against the reference
def test_two_reference_checkpoints_through_detect_multi_backend(dev, golden_dir):
    """DetectMultiBackend([a.pt, b.pt]) against the reference's attempt_load([a, b])(x)[0] (tests/golden/ensemble.pt): fp32 with the tolerance
    test_reference_checkpoint_fixture_runs_on_gpu uses for one such checkpoint, fp16 within the half-precision bounds"""
    from yolov3_amd import DetectMultiBackend, Ensemble

    gold = torch.load(golden_dir / "ensemble.pt")
    x = torch.rand(2, 3, 96, 160, generator=torch.Generator().manual_seed(9))
    assert float(x.double().abs().sum()) == gold["x_sum"]
    ws = [str(golden_dir / "ref_tiny_w025_fp16.pt"), str(golden_dir / "ref_tiny_w025_b_fp16.pt")]
    m32 = DetectMultiBackend(ws, device=dev, fp16=False)
    assert isinstance(m32.model, Ensemble) and len(m32.model) == 2 and m32.stride == 32 and m32.names == gold["names"] and not m32.fp16
    y = m32(x.to(dev))
    assert isinstance(y, list) and y[1] is None and y[0].shape == gold["pred"].shape
    torch.testing.assert_close(y[0].cpu(), gold["pred"], rtol=1e-4, atol=2e-4)
    m16 = DetectMultiBackend(ws, device=dev, fp16=True)
    m16.warmup(imgsz=(1, 3, 64, 64))
    y16 = m16(x.to(dev))[0]
    assert y16.dtype == torch.float16 and y16.shape == gold["pred"].shape
    rms, mx, corr = rel_errors(y16.float().cpu(), gold["pred"])
    print(f"[ensemble fp16 vs reference] rel RMS {rms:.5f}  max/range {mx:.5f}  corr {corr:.7f}")
    assert rms < HALF_F16["rms"] and mx < HALF_F16["mx"] and corr > HALF_F16["corr"], (rms, mx, corr)


# ------------------------------------------------------------------------------------------------ 3: one NMS over both windows
def test_one_nms_over_both_windows(dev, golden_dir):
    """The ensemble's prediction through the HIP NMS equals the oracle's NMS of the same tensor (ties in the documented stable order), and the kept rows come
    from both members' windows."""
    from yolov3_amd import attempt_load, non_max_suppression, xywh2xyxy

    ens = attempt_load([str(golden_dir / "ref_tiny_w025_fp16.pt"), str(golden_dir / "ref_tiny_w025_b_fp16.pt")], device=dev)
    shift_biases(list(ens))
    x = torch.rand(2, 3, 96, 160, generator=torch.Generator().manual_seed(9)).to(dev)
    y = ens(x)[0]
    assert y.shape == (2, 450, 85)
    got = non_max_suppression(y, 0.25, 0.45)
    want = yo.non_max_suppression(y.cpu(), 0.25, 0.45)
    box = xywh2xyxy(y[..., :4]).cpu()
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape and torch.equal(a.cpu(), b), i
        src = [(box[i] == r[:4]).all(1).nonzero().flatten().tolist() for r in a.cpu()]
        assert all(len(s) >= 1 for s in src)
        first, second = sum(1 for s in src if s[0] < 225), sum(1 for s in src if s[0] >= 225)
        print(f"[ensemble nms] image {i}: {len(src)} kept, {first} from the first member's window, {second} from the second's")
        assert first >= 20 and second >= 20, (first, second)


# ------------------------------------------------------------------------------------------------ 4: y3_label_rows
def torch_label_rows(pred, labels, n_rows):
    """the construction of general.non_max_suppression before y3_label_rows (utils/general.py:689-695)"""
    bs, _, no = pred.shape
    v = torch.zeros(bs, n_rows, no, dtype=pred.dtype, device=pred.device)
    for xi, lb in enumerate(labels):
        if len(lb):
            lb = lb.to(pred.device)
            k = len(lb)
            v[xi, :k, :4] = lb[:, 1:5].to(pred.dtype)
            v[xi, :k, 4] = 1.0
            v[xi, torch.arange(k, device=pred.device), lb[:, 0].long() + 5] = 1.0
    return v


@pytest.mark.parametrize("nc", [2, 80])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16], ids=["fp32", "fp16", "bf16"])
def test_label_rows_window_is_bit_equal_to_the_torch_construction(dev, dtype, nc):
    from yolov3_amd import ops

    no, bs, counts, w, h = nc + 5, 3, (0, 1, 5), 160.0, 96.0
    g = torch.Generator().manual_seed(nc)
    img = torch.tensor([i for i, c in enumerate(counts) for _ in range(c)], dtype=torch.float32)
    cls = torch.tensor([nc - 1, 0, nc - 1, 1, 0, nc // 2], dtype=torch.float32)
    targets = torch.cat((img[:, None], cls[:, None], torch.rand(6, 4, generator=g)), 1)
    offs = torch.tensor([0, 0, 1, 6], dtype=torch.int32)
    row0, n_rows, back = 11, 5, 3
    pred0 = torch.rand(bs, row0 + n_rows + back, no, generator=g).to(dev).to(dtype)
    pred = pred0.clone()
    ops.label_rows(pred, row0, n_rows, targets.to(dev), offs.to(dev), w, h)
    px = targets.clone()
    px[:, 2:] *= torch.tensor((w, h, w, h))            # val.py:371
    lb = [px[px[:, 0] == i, 1:] for i in range(bs)]    # val.py:372
    assert torch.equal(pred[:, row0:row0 + n_rows], torch_label_rows(pred0, lb, n_rows))
    assert torch.equal(pred[:, :row0], pred0[:, :row0]) and torch.equal(pred[:, row0 + n_rows:], pred0[:, row0 + n_rows:])
    # a class outside [0, nc) writes no one-hot element: xywh and objectness as usual, every class score 0
    out = targets.clone()
    out[:, 1] = torch.tensor([nc, -1, nc + 7, 1e9, -3, nc - 1], dtype=torch.float32)
    pred = pred0.clone()
    ops.label_rows(pred, row0, n_rows, out.to(dev), offs.to(dev), w, h)
    win = pred[:, row0:row0 + n_rows].float().cpu()
    assert (win[:, :, 5:].sum((1, 2)) == torch.tensor([0.0, 0.0, 1.0])).all() and win[2, 4, 5 + nc - 1] == 1 and (win[2, :, 4] == 1).all() and (win[1, 0, 4] == 1)
    with pytest.raises(ValueError):
        ops.label_rows(pred, row0 + back + 1, n_rows, out.to(dev), offs.to(dev), w, h)


def test_nms_with_labels_returns_what_it_returned(dev, golden_dir):
    """non_max_suppression(labels=...) on top of y3_label_rows: the reference's golden of test_nms_labels_vs_reference_golden; the oracle on a ragged fp32 case (an
    image without labels, labels on the CPU and on the device); and in every dtype exactly what the NMS returns for the prediction widened by the torch construction
    this package used before.  (A half prediction is compared with that construction alone: the reference's `torch.cat((x, v), 0)` promotes it to fp32 there, which
    this package never did.)"""
    from yolov3_amd import non_max_suppression

    rec = torch.load(golden_dir / "nms.pt")["labels"]
    pred = yo.synth_predictions(bs=2, n_rows=800, nc=80, seed=10)
    res = non_max_suppression(pred.to(dev), 0.25, 0.45, labels=rec["lb"])
    for a, b in zip(res, rec["out"]):
        assert torch.equal(canon(a), canon(b))
    g = torch.Generator().manual_seed(4)
    lb = [torch.zeros(0, 5), torch.tensor([[79.0, 300.0, 200.0, 50.0, 80.0]]),
          torch.cat((torch.randint(0, 80, (5, 1), generator=g).float(), torch.rand(5, 2, generator=g) * 500 + 60, torch.rand(5, 2, generator=g) * 100 + 10), 1)]
    for dtype in (torch.float32, torch.float16, torch.bfloat16):
        pred = yo.synth_predictions(bs=3, n_rows=500, nc=80, seed=11, dtype=torch.float16 if dtype == torch.float16 else torch.float32).to(dtype)
        before = non_max_suppression(torch.cat((pred.to(dev), torch_label_rows(pred.to(dev), lb, 5)), 1), 0.25, 0.45)
        assert sum(len(b) for b in before) > 6
        for labels in (lb, [t.to(dev) for t in lb]):
            got = non_max_suppression(pred.to(dev), 0.25, 0.45, labels=labels)
            assert len(got) == 3 and all(torch.equal(a, b) for a, b in zip(got, before)), dtype
        if dtype == torch.float32:
            want = yo.non_max_suppression(pred, 0.25, 0.45, labels=lb)
            for a, b in zip(before, want):
                assert a.shape == b.shape and torch.equal(canon(a), canon(b))


# ------------------------------------------------------------------------------------------------ 5: run_batches
_BATCHES = {}


def val_batches(model, dev, seed=6):
    """three batches of 2 at 64 x 64 in the loader's format; label counts per image (0, 3), (2, 1), (4, 0).  Random labels match nothing (every result 0), so the
    labels are the model's own most confident detections with the box shrunk by 1 / 0.9 / 0.8 / 0.7: IoUs of 1 ... 0.49 with that detection, hits at some thresholds"""
    from yolov3_amd import non_max_suppression

    if seed in _BATCHES:
        return _BATCHES[seed]
    g = torch.Generator().manual_seed(seed)
    shapes = [((64, 64), ((1.0, 1.0), (0.0, 0.0)))] * 2
    out = []
    for counts in ((0, 3), (2, 1), (4, 0)):
        im = torch.rand(2, 3, 64, 64, generator=g)
        with torch.no_grad():
            dets = non_max_suppression(model(im.to(dev))[0], 0.25, 0.45)
        rows = []
        for i, c in enumerate(counts):
            d = dets[i][:c].float().cpu()
            assert d.shape[0] == c
            for k, r in enumerate(d):
                f = (1.0, 0.9, 0.8, 0.7)[k % 4]
                rows.append([float(i), float(r[5]), float(r[0] + r[2]) / 2 / 64, float(r[1] + r[3]) / 2 / 64, float(r[2] - r[0]) * f / 64, float(r[3] - r[1]) * f / 64])
        out.append((im, torch.tensor(rows, dtype=torch.float32), shapes))
    _BATCHES[seed] = out
    return out


def hand_loop(model, batches, dev, nc, augment=False, hybrid=False, conf_thres=0.001, iou_thres=0.6):
    """val.py:351-428 over the public pieces, per image; (mp, mr, map50, map) with the stable order the package documents"""
    from yolov3_amd import metrics, non_max_suppression, process_batch, scale_boxes, xywh2xyxy

    iouv = torch.linspace(0.5, 0.95, 10, device=dev)
    stats = []
    for im, targets, shp in batches:
        im = im.to(dev).to(next(model.parameters()).dtype)
        h, w = im.shape[2:]
        out = model(im, augment=True) if augment else model(im)
        pred = out[0]
        targets = targets.to(dev).clone()
        targets[:, 2:] *= torch.tensor((w, h, w, h), device=dev)
        lb = [targets[targets[:, 0] == i, 1:] for i in range(im.shape[0])] if hybrid else []
        for si, det in enumerate(non_max_suppression(pred, conf_thres, iou_thres, labels=lb, multi_label=True, max_det=300)):
            labels = targets[targets[:, 0] == si, 1:]
            correct = torch.zeros(det.shape[0], 10, dtype=torch.bool, device=dev)
            if det.shape[0] == 0:
                if labels.shape[0]:
                    stats.append((correct.cpu().numpy(), np.zeros(0, np.float32), np.zeros(0, np.float32), labels[:, 0].cpu().numpy()))
                continue
            predn = det.clone()
            scale_boxes((h, w), predn[:, :4], shp[si][0], shp[si][1])
            if labels.shape[0]:
                tbox = scale_boxes((h, w), xywh2xyxy(labels[:, 1:5]), shp[si][0], shp[si][1])
                correct = process_batch(predn, torch.cat((labels[:, 0:1], tbox), 1), iouv)
            stats.append((correct.cpu().numpy(), det[:, 4].cpu().numpy(), det[:, 5].cpu().numpy(), labels[:, 0].cpu().numpy()))
    cols = [np.concatenate(c, 0) for c in zip(*stats)]
    if not cols[0].any():
        return (0.0, 0.0, 0.0, 0.0), cols[0].shape[0]
    _, _, p, r, _, ap, _ = metrics.ap_per_class(*cols, stable=True)
    return (float(p.mean()), float(r.mean()), float(ap[:, 0].mean()), float(ap.mean(1).mean())), cols[0].shape[0]


@pytest.fixture(scope="module")
def val_model(dev):
    m = build_model("yolov3-tiny", 80, 43, dev, torch.float32)
    shift_biases([m], seed=7)
    m.hyp = dict(HYP)
    return m


TOL = 1e-12   # tests/test_val_stats_gpu.py: the device statistics against the host mirror, fp64 curves in the same operation order


def test_run_batches_defaults_save_hybrid_and_augment_equal_the_hand_loop(dev, val_model):
    from yolov3_amd import run_batches

    batches = val_batches(val_model, dev)
    with torch.no_grad():
        res = run_batches(val_model, batches, 80)
        assert len(res) == 3 and len(res[0]) == 4 and res[0][2] > 0      # (a run without a hit compares nothing)
        want, n = hand_loop(val_model, batches, dev, 80)
        assert res[2].n == n and max(abs(a - b) for a, b in zip(res[0], want)) <= TOL, (res[0], want)
        base = res[0]
        for kw, hkw in ((dict(save_hybrid=True), dict(hybrid=True)), (dict(augment=True), dict(augment=True)), (dict(augment=True, save_hybrid=True), dict(augment=True, hybrid=True))):
            res = run_batches(val_model, batches, 80, **kw)
            want, n = hand_loop(val_model, batches, dev, 80, **hkw)
            print(f"[run_batches {kw}] {res[0]}  hand loop {want}  rows {res[2].n}")
            assert len(res[0]) == 4 and res[2].n == n and max(abs(a - b) for a, b in zip(res[0], want)) <= TOL, (kw, res[0], want)
            if "save_hybrid" in kw:
                assert res[0][3] > base[3]     # every label is its own detection of confidence 1: hits at every threshold
        # targets that are already on the device: the window is as high as the whole batch's labels, with the same results
        on_dev = [(im, t.to(dev), s) for im, t, s in batches]
        res_dev = run_batches(val_model, on_dev, 80, save_hybrid=True)
        res_cpu = run_batches(val_model, batches, 80, save_hybrid=True)
        assert res_dev[0] == res_cpu[0] and res_dev[2].n == res_cpu[2].n


def test_run_batches_compute_loss_appends_the_mean_validation_losses(dev, val_model):
    """res[4:7] == the mean of the per-batch compute_loss(model(im)[1], targets)[1]: the same kernels on the same inputs in the same order, summed on the device in
    the same order and divided once on the host as val.py:449 does -- bit for bit"""
    from yolov3_amd import ComputeLoss, Ensemble, run_batches

    batches = val_batches(val_model, dev)
    crit = ComputeLoss(val_model)
    with torch.no_grad():
        total = torch.zeros(3, device=dev)
        for im, targets, _ in batches:
            total += crit(val_model(im.to(dev))[1], targets.to(dev))[1]
        want = (total.cpu() / len(batches)).tolist()
        plain = run_batches(val_model, batches, 80)
        res = run_batches(val_model, batches, 80, compute_loss=crit, augment=True)      # (augment is ignored next to compute_loss, val.py:364)
        assert len(res[0]) == 7 and res[0][:4] == plain[0] and list(res[0][4:7]) == want and all(v > 0 for v in want), (res[0], want)
        both = run_batches(val_model, batches, 80, compute_loss=crit, save_hybrid=True)
        assert list(both[0][4:7]) == want and both[0][:4] == run_batches(val_model, batches, 80, save_hybrid=True)[0]
        with pytest.raises(TypeError, match="Ensemble"):
            run_batches(Ensemble([val_model, val_model]), batches, 80, compute_loss=crit)


def test_an_ensemble_through_run_batches_and_detect_batches_equals_the_hand_loop(dev, val_model):
    from yolov3_amd import Ensemble, detect_batches, non_max_suppression, run_batches

    other = build_model("yolov3-tiny", 80, 44, dev, torch.float32)
    shift_biases([other], seed=8)
    ens = Ensemble([val_model, other])
    batches = val_batches(val_model, dev)
    with torch.no_grad():
        for kw, hkw in ((dict(), dict()), (dict(save_hybrid=True), dict(hybrid=True))):
            res = run_batches(ens, batches, 80, **kw)
            want, n = hand_loop(ens, batches, dev, 80, **hkw)
            assert res[2].n == n and max(abs(a - b) for a, b in zip(res[0], want)) <= TOL, (kw, res[0], want)
        # half= is set on, and restored for, every member
        res16 = run_batches(ens, batches, 80, half=True)
        assert all("infer_dtype" not in m.__dict__ for m in ens) and len(res16[0]) == 4
        for augment in (False, True):
            got = list(detect_batches(ens, [b[0].to(dev) for b in batches], augment=augment))
            for dets, (im, _, _) in zip(got, batches):
                want = non_max_suppression(ens(im.to(dev), augment=augment)[0], 0.25, 0.45)
                assert len(dets) == len(want) and all(torch.equal(a, b) for a, b in zip(dets, want))
