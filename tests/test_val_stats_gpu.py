"""GPU tests of the device-side validation statistics (csrc/val_stats.hip): ap_per_class / ConfusionMatrix on the MI355X against the fixtures of the
unmodified reference (tests/golden/val_stats.pt), the tie rule against the host mirror, ValStats over ragged batches, COCO-val scale, and the
validation loop `run_batches` against a per-image val.py-style loop."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests"))

import val_stats_cases as vc  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-12


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


def _to_dev(case, dev):
    tp, conf, pc, tc = case
    return torch.from_numpy(tp).to(dev), torch.from_numpy(conf).to(dev), torch.from_numpy(pc).to(dev), torch.from_numpy(tc).to(dev)


def _compare(got, want, what, exact=False):
    assert len(got) == len(want) == 7
    worst = 0.0
    for i, (a, b) in enumerate(zip(got, want)):
        a, b = np.asarray(a), np.asarray(b)
        assert a.shape == b.shape, (what, i, a.shape, b.shape)
        d = float(np.abs(a.astype(np.float64) - b.astype(np.float64)).max(initial=0.0))
        worst = max(worst, d)
        if exact or i in (0, 1, 6):
            assert np.array_equal(a, b), (what, i, d)   # integer counts, class ids
        else:
            assert d <= TOL, (what, i, d)
    print(f"[val stats] {what}: max |diff| {worst:.3e}")


def test_ap_per_class_device_matches_the_reference_goldens(dev, golden_dir):
    from yolov3_amd import metrics

    gold = torch.load(golden_dir / "val_stats.pt")["ap"]
    assert list(gold) == vc.AP_CASES
    for name in vc.AP_CASES:
        case = vc.ap_case(name)
        got = metrics.ap_per_class_device(*_to_dev(case, dev))
        want = [t.numpy() for t in gold[name]["out"]]
        _compare(got, want, name)
        # the chosen confidence index: p / r / f1 are read at it, so a different index would show above; the host mirror picks the same one
        assert all(g.dtype == np.float64 for g in got[:6]) and got[6].dtype.kind == "i"


def test_score_ties_follow_arrival_order_and_repeat_bitwise(dev):
    from yolov3_amd import metrics

    case = vc.tied_ap_case()
    want = metrics.ap_per_class(*case, stable=True)
    a = metrics.ap_per_class_device(*_to_dev(case, dev))
    b = metrics.ap_per_class_device(*_to_dev(case, dev))
    _compare(a, want, "ties vs host stable=True")
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()


def test_valstats_ragged_batches_equal_the_concatenated_rows(dev):
    """counts 0, 1 and max_det, images with labels and no detections and the reverse, several reallocations: the same bits as ap_per_class_device
    on the concatenated rows (and as the host mirror within 1e-12)"""
    from yolov3_amd import metrics

    g = torch.Generator().manual_seed(5)
    nc, T, max_det = 7, 10, 300
    st = metrics.ValStats(nc, torch.linspace(0.5, 0.95, T), dev)
    cat = [[], [], [], []]
    caps = set()
    for b in range(40):
        bs = int(torch.randint(1, 9, (1,), generator=g))
        counts = [int(torch.randint(0, max_det + 1, (1,), generator=g)) for _ in range(bs)]
        counts[0] = (0, 1, max_det)[b % 3]
        rows = torch.rand(bs, max_det, 6, generator=g)
        rows[:, :, 4] = (rows[:, :, 4] * 512).round() / 512          # some score ties across batches
        rows[:, :, 5] = torch.randint(0, nc, (bs, max_det), generator=g).float()
        correct = (torch.rand(bs, max_det, 1, generator=g) * (0.4 + rows[:, :, 4:5]) > torch.linspace(0.5, 1.2, T)[None, None, :]).to(torch.uint8)
        nl = [int(torch.randint(0, 5, (1,), generator=g)) for _ in range(bs)]
        if b % 4 == 0:
            nl[0] = 3 if counts[0] == 0 else 0   # labels without detections / detections without labels
        labels = torch.cat((torch.randint(0, nc, (sum(nl), 1), generator=g).float(), torch.rand(sum(nl), 4, generator=g)), 1)
        offs = torch.tensor([0, *np.cumsum(nl)], dtype=torch.int32)
        st.update(rows.to(dev), torch.tensor(counts, dtype=torch.int32, device=dev), counts, correct.to(dev), labels.to(dev), offs.to(dev))
        caps.add(st._cap)
        for i, c in enumerate(counts):
            cat[0].append(correct[i, :c].bool())
            cat[1].append(rows[i, :c, 4])
            cat[2].append(rows[i, :c, 5])
        cat[3].append(labels[:, 0])
    tp, conf, pc, tc = (torch.cat(c) for c in cat)
    assert st.n == conf.shape[0] and len(caps) >= 4, (st.n, caps)
    assert np.array_equal(st.nt, np.bincount(tc.numpy().astype(int), minlength=nc))
    got = st.compute()
    _compare(got, metrics.ap_per_class_device(tp.to(dev), conf.to(dev), pc.to(dev), tc.to(dev), nc=nc), "ragged vs concatenated", exact=True)
    want = metrics.ap_per_class(tp.numpy(), conf.numpy(), pc.numpy(), tc.numpy(), stable=True)
    _compare(got, want, "ragged vs host stable=True")
    mp, mr, m50, m = st.results()
    assert max(abs(mp - want[2].mean()), abs(mr - want[3].mean()), abs(m50 - want[5][:, 0].mean()), abs(m - want[5].mean(1).mean())) <= TOL
    maps = st.maps(nc)
    assert maps.shape == (nc,) and all(abs(maps[c] - want[5][i].mean()) <= TOL for i, c in enumerate(want[6]))
    # an empty run, and a run without a correct detection: zeros (val.py:425)
    empty = metrics.ValStats(nc, T, dev)
    assert empty.results() == (0.0, 0.0, 0.0, 0.0) and empty.compute()[5].shape == (0, T)
    none = metrics.ValStats(nc, T, dev)
    none.append_rows(torch.zeros(20, T, dtype=torch.bool, device=dev), torch.rand(20, device=dev), torch.zeros(20, device=dev))
    none.add_labels(torch.zeros(4, device=dev))
    assert none.results() == (0.0, 0.0, 0.0, 0.0) and np.array_equal(none.maps(nc), np.zeros(nc))


def test_coco_val_scale_matches_the_host_mirror(dev):
    """1.5 M rows (5000 images x 300 detections), 80 classes, T = 10; class 0 owns about a quarter of the rows"""
    from yolov3_amd import metrics

    case = vc.coco_scale_case()
    assert case[0].shape == (1_500_000, 10)
    want = metrics.ap_per_class(*case, stable=True)
    got = metrics.ap_per_class_device(*_to_dev(case, dev), nc=80)
    _compare(got, want, "coco scale")
    assert float(want[5].mean()) > 0.0


def test_confusion_matrix_matches_the_reference_golden(dev, golden_dir):
    from yolov3_amd import metrics

    gold = torch.load(golden_dir / "val_stats.pt")["confusion"]
    want = gold["matrix"].numpy()
    imgs = vc.confusion_images()
    per_image = metrics.ConfusionMatrix(gold["nc"], gold["conf"], gold["iou_thres"])
    for det, lab in imgs:                       # val.py:386-406
        if det.shape[0] == 0:
            if lab.shape[0]:
                per_image.process_batch(None, lab[:, 0].to(dev))
            continue
        if lab.shape[0]:
            per_image.process_batch(det.to(dev), lab.to(dev))
    assert per_image.matrix.dtype == np.float64 and np.array_equal(per_image.matrix, want), per_image.matrix - want
    batched = metrics.ConfusionMatrix(gold["nc"], gold["conf"], gold["iou_thres"])
    for lo in range(0, len(imgs), 5):           # batches of 5, 5 and 4 images
        part = imgs[lo:lo + 5]
        max_det = max(max(d.shape[0] for d, _ in part), 1) + 2
        rows = torch.full((len(part), max_det, 6), 7.0)       # rows beyond the counts hold junk that would match if it were read
        for i, (d, _) in enumerate(part):
            rows[i, :d.shape[0]] = d
        counts = torch.tensor([d.shape[0] for d, _ in part], dtype=torch.int32)
        labels = torch.cat([l for _, l in part])
        offs = torch.tensor([0, *np.cumsum([l.shape[0] for _, l in part])], dtype=torch.int32)
        batched.process_batch_batched(rows.to(dev), counts.to(dev), labels.to(dev), offs.to(dev))
    assert np.array_equal(batched.matrix, want), batched.matrix - want
    tp, fp = batched.tp_fp()
    assert np.array_equal(tp, want.diagonal()[:-1]) and np.array_equal(fp, (want.sum(1) - want.diagonal())[:-1])


def test_run_batches_equals_the_per_image_loop_without_extra_synchronisation(dev, monkeypatch):
    """`run_batches` on the synthetic scenes of tests/map_parity.py (a briefly trained yolov3-tiny, fp16) against the per-image loop of val.py
    (NMS, scale_boxes, process_batch per image, three `.cpu()` per image, host ap_per_class with stable=True); and between the first batch and the
    final read-back the only host read is the NMS counts (`Tensor.tolist` in ops.nms_raw)."""
    import copy

    import map_parity as mp
    from yolov3_amd import ConfusionMatrix, metrics, non_max_suppression, process_batch, run_batches, scale_boxes, xywh2xyxy

    hw, nc, bs = 128, 3, 16
    train_x, train_l = mp.make_scenes(96, hw, nc, seed=1)
    val_x, val_l = mp.make_scenes(40, hw, nc, seed=2)
    model, _ = mp.train_on_gpu("yolov3-tiny", nc, hw, 300, dev, train_x, train_l)
    m = copy.deepcopy(model).half().eval()
    starts = list(range(0, val_x.shape[0], bs))       # 16 + 16 + 8 images
    shapes = [((hw, hw), ((1.0, 1.0), (0.0, 0.0)))] * bs

    def batches(log=None):
        for b in starts:
            idx = torch.arange(b, min(b + bs, val_x.shape[0]))
            if log is not None:
                log.append("batch")
            yield val_x[idx], mp.batch_targets(val_l, idx), shapes[:len(idx)]

    # the per-image loop
    iouv = torch.linspace(0.5, 0.95, 10, device=dev)
    stats, cm_ref = [], ConfusionMatrix(nc)
    with torch.no_grad():
        for im, targets, shp in batches():
            pred = m(im.to(dev).half())[0]
            targets = targets.to(dev)
            targets[:, 2:] *= torch.tensor((hw, hw, hw, hw), device=dev)
            for si, det in enumerate(non_max_suppression(pred, 0.001, 0.6, multi_label=True, max_det=300)):
                labels = targets[targets[:, 0] == si, 1:]
                correct = torch.zeros(det.shape[0], 10, dtype=torch.bool, device=dev)
                if det.shape[0] == 0:
                    if labels.shape[0]:
                        stats.append((correct.cpu().numpy(), np.zeros(0, np.float32), np.zeros(0, np.float32), labels[:, 0].cpu().numpy()))
                        cm_ref.process_batch(None, labels[:, 0])
                    continue
                predn = det.clone()
                scale_boxes((hw, hw), predn[:, :4], shp[si][0], shp[si][1])
                if labels.shape[0]:
                    tbox = scale_boxes((hw, hw), xywh2xyxy(labels[:, 1:5]), shp[si][0], shp[si][1])
                    labelsn = torch.cat((labels[:, 0:1], tbox), 1)
                    correct = process_batch(predn, labelsn, iouv)
                    cm_ref.process_batch(predn, labelsn)
                stats.append((correct.cpu().numpy(), det[:, 4].cpu().numpy(), det[:, 5].cpu().numpy(), labels[:, 0].cpu().numpy()))
    cols = [np.concatenate(c, 0) for c in zip(*stats)]
    assert cols[0].shape[0] > 0
    _, _, p, r, _, ap, _ = metrics.ap_per_class(*cols, stable=True)
    want = (float(p.mean()), float(r.mean()), float(ap[:, 0].mean()), float(ap.mean(1).mean())) if cols[0].any() else (0.0, 0.0, 0.0, 0.0)

    log = []
    for name in ("cpu", "item", "tolist", "numpy"):
        orig = getattr(torch.Tensor, name)

        def counted(self, *a, _orig=orig, _name=name, **k):
            if self.is_cuda:
                log.append(_name)
            return _orig(self, *a, **k)

        monkeypatch.setattr(torch.Tensor, name, counted)
    with torch.no_grad():
        got, maps, st, cm = run_batches(m, batches(log), nc, confusion=True)
        log.append("returned")
    monkeypatch.undo()
    print("[val stats] run_batches", got, "per-image loop", want, "rows", st.n, "host reads", log)
    assert st.n == cols[0].shape[0]
    assert max(abs(a - b) for a, b in zip(got, want)) <= TOL, (got, want)
    assert np.array_equal(cm.matrix, cm_ref.matrix)
    assert np.array_equal(st.nt, np.bincount(cols[3].astype(int), minlength=nc))
    last_batch = max(i for i, e in enumerate(log) if e == "batch")
    first = log.index("batch")
    loop = [e for e in log[first:last_batch] if e != "batch"]
    assert loop and set(loop) == {"tolist"} and len(loop) <= 3 * (len(starts) - 1), log      # the NMS counts (at most three attempts per batch), nothing else
    tail = [e for e in log[last_batch + 1:log.index("returned")]]
    assert [e for e in tail if e != "tolist"] == ["cpu"], log                                  # after the last batch: its NMS counts, then ONE read-back of the result block
