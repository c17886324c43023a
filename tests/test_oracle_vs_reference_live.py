"""The oracle against the UNMODIFIED reference on more seeded cases than tests/test_oracle_golden.py holds -- a wider pin: 120 val
matches, 60 letterbox geometries, 4 NMS regimes, 8 loss heads / hyp variants, 2 x 3 autobalance calls.  The reference's outputs on these
cases are recorded in tests/golden/reference_cases.pt (tests/golden/make_golden.py cases); the inputs are regenerated here from the same
seeds and checked against the recorded checksums.  tests/golden/class_counts.pt (tests/golden/make_class_counts_golden.py) adds
ComputeLoss on heads with 1, 2, 3 and 60 classes and Detect with 1 and 2.  CPU only."""
import pytest
import torch
import yaml
from pathlib import Path

from oracle import yolo_oracle as yo

CFG = Path(__file__).resolve().parents[1] / "yolov3_amd" / "cfg"


def checksum(t):
    return float(t.double().abs().sum())


def dense(g):
    """a gradient recorded as (shape, flat indices of its non-zeros, their values)"""
    t = torch.zeros(g["shape"], dtype=g["val"].dtype).reshape(-1)
    t[g["idx"].long()] = g["val"]
    return t.reshape(g["shape"])


@pytest.fixture(scope="module")
def ref(golden_dir):
    return torch.load(golden_dir / "reference_cases.pt")


def test_process_batch_oracle_equals_reference_on_many_cases(ref):
    """val.process_batch (reference val.py:147-188) == oracle.process_batch on 120 seeded images: label counts 1-29, 20-139
    detections, 1-6 classes, three duplicate regimes (several detections per label)."""
    iouv = torch.linspace(0.5, 0.95, 10)
    checked = 0
    assert len(ref["process_batch"]) == 120
    for seed, rec in enumerate(ref["process_batch"]):
        det, lab = yo.synth_val_case(seed + 1000, n_lab=1 + seed % 29, n_det=20 + seed, nc=1 + seed % 6, dup=(seed % 3) / 2)
        assert checksum(det) == rec["det_sum"] and checksum(lab) == rec["lab_sum"], f"input drift, seed {seed}"
        want = rec["want"]
        got = yo.process_batch(det, lab, iouv)
        assert torch.equal(got, want), f"seed {seed}"
        checked += int(want.sum())
    assert checked > 1000


def test_scale_boxes_oracle_equals_reference_on_many_shapes(ref):
    """utils.general.scale_boxes (reference :613-626) == oracle.scale_boxes, bit-exact, over letterbox geometries derived the way
    val.py / detect.py derive them (ratio_pad None and the dataloader's (ratio, pad) form)."""
    g = torch.Generator().manual_seed(0)
    assert len(ref["scale_boxes"]) == 60
    for i, rec in enumerate(ref["scale_boxes"]):
        h0, w0 = int(torch.randint(120, 1400, (1,), generator=g)), int(torch.randint(120, 1400, (1,), generator=g))
        s1 = (int(torch.randint(5, 21, (1,), generator=g)) * 32, int(torch.randint(5, 21, (1,), generator=g)) * 32)
        boxes = yo.synth_scale_case(s1, seed=20 + i, n=64)
        rp = None
        if i % 2:
            r = min(s1[0] / h0, s1[1] / w0)
            rp = ((r, r), ((s1[1] - round(w0 * r)) / 2, (s1[0] - round(h0 * r)) / 2))
        assert (s1, (h0, w0), rp) == (tuple(rec["s1"]), tuple(rec["s0"]), rec["ratio_pad"]) and checksum(boxes) == rec["boxes_sum"], f"input drift, case {i}"
        want = rec["want"]
        got = yo.scale_boxes(s1, boxes.clone()[:, :4], (h0, w0), rp)
        assert torch.equal(got, want), (i, s1, (h0, w0), rp)


def test_nms_oracle_equals_reference_on_fresh_seeds(ref):
    """non_max_suppression (reference utils/general.py:630-750, with the restated torchvision nms) == oracle on seeds the golden
    files do not hold: both regimes, agnostic and class-filtered."""
    cases = [
        (dict(bs=2, n_rows=1800, nc=80, seed=101), dict(conf_thres=0.001, iou_thres=0.6, multi_label=True, max_det=300)),
        (dict(bs=2, n_rows=1800, nc=80, seed=102), dict(conf_thres=0.25, iou_thres=0.45)),
        (dict(bs=1, n_rows=1500, nc=20, seed=103, hits=0.1), dict(conf_thres=0.05, iou_thres=0.5, agnostic=True)),
        (dict(bs=1, n_rows=1500, nc=8, seed=104, n_gt=30), dict(conf_thres=0.1, iou_thres=0.45, classes=[1, 4])),
    ]
    assert len(ref["nms"]) == len(cases)
    for (gk, nk), rec in zip(cases, ref["nms"]):
        assert (gk, nk) == (rec["gen"], rec["nms"])
        pred = yo.synth_predictions(**gk)
        assert checksum(pred) == rec["pred_sum"], f"input drift, {gk}"
        want = rec["want"]
        got = yo.non_max_suppression(pred, **nk)
        assert len(got) == len(want)
        for a, b in zip(got, want):
            assert a.shape == b.shape and torch.equal(a, b), (gk, nk)


def test_compute_loss_oracle_equals_reference_on_fresh_targets(ref):
    """ComputeLoss (reference utils/loss.py:98-244) == oracle.compute_loss -- value, items and d loss / d predictions -- on target
    sets the golden file does not hold: 8 seeds, focal / label-smoothing / pos_weight variants, yolov3 and yolov3-tiny heads, the last four with sort_obj_iou and duplicated cells."""
    variants = [dict(), dict(fl_gamma=1.5), dict(label_smoothing=0.1, cls_pw=0.8, obj_pw=1.3)]
    heads = [("yolov3", 80, 96, 2), ("yolov3-tiny", 20, 128, 3), ("yolov3", 5, 64, 4), ("yolov3-tiny", 80, 96, 2)] * 2
    assert len(ref["loss"]) == len(heads)
    for i, ((name, nc, hw, bs), rec) in enumerate(zip(heads, ref["loss"])):
        assert tuple(rec["head"]) == (name, nc, hw, bs)
        d = yaml.safe_load(open(CFG / f"{name}.yaml"))
        layers, save, anchors, nc_v = yo.parse_cfg(d, 3, nc)
        strides = yo.model_strides(layers)
        hyp = dict(box=0.05, cls=0.5, cls_pw=1.0, obj=1.0, obj_pw=1.0, anchor_t=4.0, fl_gamma=0.0, label_smoothing=0.0)
        hyp.update(variants[i % len(variants)])
        nl = len(strides)
        hyp["box"] *= 3 / nl
        hyp["cls"] *= nc / 80 * 3 / nl
        hyp["obj"] *= (hw / 640) ** 2 * 3 / nl
        assert hyp == rec["hyp"], i
        sort_iou = i >= 4   # the second pass over the four heads: ComputeLoss.sort_obj_iou (utils/loss.py:101,156-158)
        assert sort_iou == rec["sort_obj_iou"]
        shapes = [(bs, 3, hw // int(s), hw // int(s), nc + 5) for s in strides]
        tg = yo.synth_targets(bs, nc, seed=70 + i)
        if sort_iou:   # duplicate cells with different boxes, so that the order of the writes matters
            tg = torch.cat((tg, tg[: max(1, tg.shape[0] // 3)] * torch.tensor([1, 1, 1, 1, 0.8, 1.25])))
        assert checksum(tg) == rec["tg_sum"], f"input drift, head {i}"
        p = [t.requires_grad_(True) for t in yo.synth_raw_predictions(shapes, seed=50 + i)]
        assert sum(checksum(t.detach()) for t in p) == rec["p_sum"], f"input drift, head {i}"
        loss, items, _ = yo.compute_loss(p, tg, rec["anchors"].clone(), hyp, nc, sort_obj_iou=sort_iou)
        loss.backward()
        torch.testing.assert_close(loss, rec["loss"], rtol=1e-6, atol=1e-6)
        torch.testing.assert_close(items, rec["items"], rtol=1e-6, atol=1e-6)
        assert len(p) == len(rec["grads"])
        for a, b in zip(p, rec["grads"]):
            torch.testing.assert_close(a.grad, dense(b), rtol=1e-5, atol=1e-8)


def test_autobalance_oracle_equals_reference_over_consecutive_calls(ref):
    """ComputeLoss(autobalance=True) (reference utils/loss.py:121, :171-175): the per-level objectness weights after three consecutive calls,
    and every call's loss, from the unmodified reference and from oracle.compute_loss(balance=..., autobalance_ssi=...)."""
    heads = [("yolov3", 80, 96, 2), ("yolov3-tiny", 20, 128, 3)]
    assert len(ref["autobalance"]) == len(heads)
    for (name, nc, hw, bs), rec in zip(heads, ref["autobalance"]):
        assert tuple(rec["head"]) == (name, nc, hw, bs)
        d = yaml.safe_load(open(CFG / f"{name}.yaml"))
        layers, save, anchors, nc_v = yo.parse_cfg(d, 3, nc)
        strides = yo.model_strides(layers)
        hyp = dict(box=0.05, cls=0.5, cls_pw=1.0, obj=1.0, obj_pw=1.0, anchor_t=4.0, fl_gamma=0.0, label_smoothing=0.0)
        ssi = [int(s) for s in strides].index(16)
        assert rec["ssi"] == ssi
        balance = list(rec["balance0"])
        shapes = [(bs, 3, hw // int(s), hw // int(s), nc + 5) for s in strides]
        assert len(rec["calls"]) == 3
        for step, call in enumerate(rec["calls"]):
            tg = yo.synth_targets(bs, nc, seed=90 + step)
            p = yo.synth_raw_predictions(shapes, seed=60 + step)
            loss, _, _ = yo.compute_loss(p, tg, rec["anchors"].clone(), hyp, nc, balance=balance, autobalance_ssi=ssi)
            torch.testing.assert_close(loss, call["loss"], rtol=1e-6, atol=1e-6)
            torch.testing.assert_close(torch.tensor(balance), torch.tensor(call["balance"]), rtol=1e-6, atol=1e-7)
        assert abs(balance[ssi] - 1.0) < 1e-9 and balance != [4.0, 1.0, 0.4][: len(balance)]


# ------------------------------------------------------------------------------------------------ class counts 1 / 2 / 3 / 60 (tests/golden/make_class_counts_golden.py)
def dense_level(g):
    """one level's gradient recorded as its objectness plane (channel 4) and the sparse rest"""
    t = dense(g["rest"])
    t[..., 4] = g["obj"]
    return t


@pytest.fixture(scope="module")
def ref_cc(golden_dir):
    return torch.load(golden_dir / "class_counts.pt")


def test_compute_loss_oracle_equals_reference_at_small_class_counts(ref_cc):
    """ComputeLoss (reference utils/loss.py:98-244) == oracle.compute_loss -- value, items and d loss / d predictions -- on yolov3-tiny heads with 1 and 2 classes
    (plain, focal, label smoothing, both) and yolov3 heads with 1, 3 and 60 classes.  One class: the reference adds no class loss (`if self.nc > 1`, :164), so items[2]
    is 0 and no class logit has a gradient."""
    import class_count_cases as cc

    heads = [("yolov3-tiny", 1, 96, 2), ("yolov3-tiny", 2, 96, 2), ("yolov3-tiny", 2, 96, 2), ("yolov3-tiny", 2, 96, 2), ("yolov3-tiny", 2, 96, 2),
             ("yolov3", 1, 64, 2), ("yolov3", 3, 64, 2), ("yolov3", 60, 64, 2)]
    overs = [{}, {}, dict(fl_gamma=1.5), dict(label_smoothing=0.1), dict(fl_gamma=1.5, label_smoothing=0.1), {}, {}, {}]
    assert [tuple(r["head"]) for r in ref_cc["loss"]] == heads and [r["over"] for r in ref_cc["loss"]] == overs
    for i, ((name, nc, hw, bs), over, rec) in enumerate(zip(heads, overs, ref_cc["loss"])):
        layers, save, anchors, nc_v = yo.parse_cfg(yaml.safe_load(open(CFG / f"{name}.yaml")), 3, nc)
        strides = yo.model_strides(layers)
        hyp = cc.scaled_hyp(len(strides), nc, hw, over)
        assert hyp == rec["hyp"], i
        shapes = [(bs, 3, hw // int(s), hw // int(s), nc + 5) for s in strides]
        seed, tg = cc.pick_targets(bs, nc, shapes, rec["anchors"], rec["tg_seed"])
        assert seed == rec["tg_seed"] and checksum(tg) == rec["tg_sum"], f"input drift, head {i}"
        assert set(tg[:, 1].long().tolist()) >= ({nc - 1} if nc > 4 else set(range(nc)))
        p = [t.requires_grad_(True) for t in yo.synth_raw_predictions(shapes, seed=rec["p_seed"])]
        assert sum(checksum(t.detach()) for t in p) == rec["p_sum"], f"input drift, head {i}"
        loss, items, _ = yo.compute_loss(p, tg, rec["anchors"].clone(), hyp, nc)
        loss.backward()
        torch.testing.assert_close(loss, rec["loss"], rtol=1e-6, atol=1e-6)
        torch.testing.assert_close(items, rec["items"], rtol=1e-6, atol=1e-6)
        assert len(p) == len(rec["grads"])
        for a, b in zip(p, rec["grads"]):
            want = dense_level(b)
            torch.testing.assert_close(a.grad, want, rtol=1e-5, atol=1e-8)
            assert (want[..., :4].abs().sum(-1) > 0).any(), "a level without a matched cell pins nothing but the objectness plane"
            if nc == 1:
                assert not a.grad[..., 5].any() and not want[..., 5].any()
        if nc == 1:
            assert float(rec["items"][2]) == 0.0 and float(items[2]) == 0.0
            torch.testing.assert_close(loss, (items[0] + items[1]).reshape(1) * bs, rtol=1e-6, atol=1e-6)


@pytest.mark.parametrize("nc,dtype", [(1, torch.float32), (1, torch.float16), (2, torch.float32), (2, torch.float16)])
def test_decode_oracle_equals_reference_at_one_and_two_classes(ref_cc, nc, dtype):
    """The eval branch of Detect (reference models/yolo.py:98-110) on yolov3-tiny's two levels with no = 6 and 7 == oracle.detect_decode."""
    gold = ref_cc["decode"][f"nc{nc}-{str(dtype).split('.')[-1]}"]
    no = nc + 5
    g = torch.Generator().manual_seed(gold["seed"])
    xs = [torch.randn(2, 3 * no, s, s + 1, generator=g) * 2.0 for s in gold["sizes"]]
    if dtype == torch.float16:
        xs = [x.half() for x in xs]
    assert sum(checksum(x) for x in xs) == gold["in_sum"], "input drift"
    raw = [x.view(2, 3, no, x.shape[2], x.shape[3]).permute(0, 1, 3, 4, 2).contiguous() for x in xs]
    z = yo.detect_decode(raw, gold["anchors_grid"].to(dtype), torch.tensor(gold["strides"]).to(dtype))
    assert z.dtype == gold["z"].dtype and z.shape == gold["z"].shape == (2, 3 * sum(s * (s + 1) for s in gold["sizes"]), no)
    if dtype == torch.float32:
        torch.testing.assert_close(z, gold["z"], rtol=1e-6, atol=1e-6)
    else:   # (every op rounded through fp16 on both sides, as tests/test_oracle_golden.py::test_decode_matches_reference holds the other class counts)
        assert torch.equal(z, gold["z"])
