"""Head-first NMS (knob nms_head, detect_nms.hip::nms_sort_kernel): round 1 orders, prepares and suppresses only a head of every image's score ranks, round 2
redoes the images that kept fewer than max_det boxes there over their full range.  The result must not depend on the head: every case is compared bit for bit --
rows, order, counts -- with the oracle (where it has the dtype and the argument) and with the same call at nms_head = 0, for heads of 64 and 128 ranks and the
default, in both forms of the head (N > 0: N ranks ordered among the candidates above a cutoff of the leading score digits; N < 0: N ranks of the full ordering).
The status word says how many images took round 2 (ops.nms_raw.last_round2): the cases built to need the fallback assert that it ran."""
import pytest
import torch

from oracle import yolo_oracle as yo

pytestmark = pytest.mark.gpu

HEADS = [64, 128, None]   # None = the default
_ORACLE = {}              # case -> the oracle's result, computed once and left unchanged


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


def _same(got, want, what):
    assert len(got) == len(want), what
    for i, (a, b) in enumerate(zip(got, want)):
        a, b = a.float().cpu(), b.float().cpu()
        assert a.shape == b.shape, f"{what} image {i}: {tuple(a.shape)} vs {tuple(b.shape)}"
        assert torch.equal(a, b), f"{what} image {i}: rows differ (first bad row {(a != b).any(1).nonzero()[:1].tolist()})"


def _oracle(key, pred, **kw):
    if key not in _ORACLE:
        _ORACLE[key] = yo.non_max_suppression(pred, **kw)
    return _ORACLE[key]


def _run(tune, pred_dev, head, conf, iou, max_det, agnostic=False, sort=1, **extra):
    """(rows per image, images that took round 2) of one ops.nms_raw call at the given knobs"""
    from yolov3_amd import ops

    head = _default_head() if head is None else head   # (resets every knob: set them after it)
    tune("nms_sort", sort)
    tune("nms_head", head)
    rows, counts = ops.nms_raw(pred_dev, conf, iou, None, agnostic, True, max_det, **extra)
    return [rows[i, :c].cpu() for i, c in enumerate(counts)], ops.nms_raw.last_round2


def _default_head():
    from yolov3_amd import ops

    ops.tune_reset()
    return ops.tune_get("nms_head")


def _candidates(pred, conf):
    """candidates per image under multi_label (x[:, 5:] * x[:, 4:5] > conf among the rows with obj > conf), in the input dtype"""
    ok = (pred[..., 5:] * pred[..., 4:5] > conf) & (pred[..., 4:5] > conf)
    return ok.flatten(1).sum(1).tolist()


# ------------------------------------------------------------------------------------------------ one batch with every kind of image
def _mixed_batch(small):
    """image 0: boxes that rarely overlap, satisfied in any head; image 1: 2700 near-duplicates of three boxes (one per class) hold the first 2700 ranks -- at most a
    few of them are kept, so no head reaches max_det; image 2: `small` candidates (fewer than any head); image 3: none"""
    g = torch.Generator().manual_seed(11)
    bs, n_rows, nc = 4, 4000, 3
    pred = torch.zeros(bs, n_rows, 5 + nc)
    pred[..., :2] = torch.rand(bs, n_rows, 2, generator=g) * 600 + 20
    pred[..., 2:4] = torch.rand(bs, n_rows, 2, generator=g) * 30 + 6
    pred[..., 4] = 1.0
    cls = torch.randint(0, nc, (bs, n_rows), generator=g)
    score = torch.rand(bs, n_rows, generator=g) * 0.6 + 0.1                  # 0.1 .. 0.7
    dup = torch.randperm(n_rows, generator=g)[:2700]                          # image 1: rows scattered over the tensor
    k = torch.arange(2700) % nc
    pred[1, dup, 0] = 100.0 + 150.0 * k + torch.rand(2700, generator=g)       # jitter below a pixel on 40 px boxes: IoU > 0.9
    pred[1, dup, 1] = 300.0 + torch.rand(2700, generator=g)
    pred[1, dup, 2:4] = 40.0
    cls[1, dup] = k
    score[1, dup] = 0.8 + 0.15 * torch.rand(2700, generator=g)                # above every other box of the image
    pred.scatter_(2, (5 + cls).unsqueeze(-1), score.unsqueeze(-1))
    pred[2, small:, 4] = 0.0
    pred[3, :, 4] = 0.0
    return pred.half()


@pytest.mark.parametrize("small", [1, 40])
def test_mixed_batch_takes_both_rounds(dev, tune, small):
    pred = _mixed_batch(small)
    kw = dict(conf_thres=0.05, iou_thres=0.6, max_det=20)
    want = _oracle(("mixed", small), pred, multi_label=True, **kw)
    assert [w.shape[0] for w in want][0] == 20 and want[2].shape[0] >= 1 and want[3].shape[0] == 0
    cand = _candidates(pred, 0.05)
    p = pred.to(dev)
    base, r2 = _run(tune, p, 0, 0.05, 0.6, 20)
    assert r2 == 0
    _same(base, want, "nms_head 0 vs oracle")
    for h in HEADS:
        for sign in (1, -1):
            hv = (_default_head() if h is None else h) * sign
            got, r2 = _run(tune, p, hv, 0.05, 0.6, 20)
            _same(got, want, f"nms_head {hv} vs oracle")
            _same(got, base, f"nms_head {hv} vs nms_head 0")
            # image 1 must take round 2 (its head holds near-duplicates only), image 0 must not (20 of its first 64 boxes are kept), images 2 and 3 cannot
            assert cand[1] > abs(hv) and r2 == 1, f"nms_head {hv}: {r2} images took round 2, candidates {cand}"


# ------------------------------------------------------------------------------------------------ the kept count against the head's last rank
def _ladder(head, max_det, where):
    """one image, one class, N = head + 100 boxes on a grid (no two overlap) with strictly falling scores, in shuffled row order; ranks 1 .. d repeat the box of
    rank 0 and are suppressed, so rank r > d is the (r - d + 1)-th kept box.  d puts the max_det-th kept box at rank head - 1 / at rank head; "never": every box
    behind rank 0 of the head is a repeat, and fewer than max_det boxes follow."""
    n = head + 100
    if where == "never":
        n, d = head + max_det - 2, head - 1
    else:
        d = max(head - max_det + (0 if where == "last" else 1), 0)
    g = torch.Generator().manual_seed(head * 7 + max_det)
    r = torch.arange(n)
    pred = torch.zeros(1, n, 7)
    pred[0, :, 0] = 10.0 + 10.0 * (r % 60)
    pred[0, :, 1] = 10.0 + 10.0 * (r // 60)
    pred[0, 1:d + 1, 0:2] = pred[0, 0, 0:2]
    pred[0, :, 2:4] = 6.0
    pred[0, :, 4] = 0.99 - 0.6 * r / n
    pred[0, :, 5] = 1.0
    kept_in_head = 1 + max(min(head, n) - 1 - d, 0)
    return pred[:, torch.randperm(n, generator=g)], int(n > head and kept_in_head < max_det), min(max_det, n - d)


@pytest.mark.parametrize("where", ["last", "behind", "never"])
@pytest.mark.parametrize("max_det", [5, 64, 65, 300])
def test_kept_count_against_the_heads_last_rank(dev, tune, max_det, where):
    for h in HEADS:
        head = _default_head() if h is None else h
        pred, need2, kept = _ladder(head, max_det, where)
        want = _oracle(("ladder", head, max_det, where), pred, conf_thres=0.25, iou_thres=0.5, multi_label=True, max_det=max_det)
        assert want[0].shape[0] == kept
        p = pred.to(dev)
        base, _ = _run(tune, p, 0, 0.25, 0.5, max_det)
        _same(base, want, "nms_head 0 vs oracle")
        got, r2 = _run(tune, p, -head, 0.25, 0.5, max_det)      # a head of exactly `head` ranks
        _same(got, want, f"nms_head {-head} max_det {max_det} {where} vs oracle")
        assert r2 == need2, f"nms_head {-head} max_det {max_det} {where}: round 2 ran for {r2} images, expected {need2}"
        got, r2 = _run(tune, p, head, 0.25, 0.5, max_det)       # the same ranks, ordered among the candidates above the digit cutoff only
        _same(got, want, f"nms_head {head} max_det {max_det} {where} vs oracle")
        assert r2 == need2, f"nms_head {head} max_det {max_det} {where}: round 2 ran for {r2} images, expected {need2}"


# ------------------------------------------------------------------------------------------------ ties, dtypes
def _ties(dtype):
    pred = yo.synth_predictions(bs=3, n_rows=4000, nc=20, seed=5, dtype=torch.float32, hits=0.3)
    pred[..., 4] = (pred[..., 4] * 8).round().div(8)        # 9 objectness levels
    pred[..., 5:] = (pred[..., 5:] * 4).round().div(4)      # 5 class-score levels: a few distinct products, thousands of exact ties across every rank and every digit cutoff
    return pred.to(dtype)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float32], ids=["fp16", "bf16", "fp32"])
def test_score_ties_across_the_head_and_the_digit_cutoff(dev, tune, dtype):
    pred = _ties(dtype)
    p = pred.to(dev)
    base, _ = _run(tune, p, 0, 0.05, 0.5, 300)
    assert sum(b.shape[0] for b in base) > 50
    if dtype == torch.bfloat16:   # (the CPU reference has no bf16 path for every op: the device sorts are the second check)
        _same(base, _run(tune, p, 0, 0.05, 0.5, 300, sort=0)[0], "own sort vs device sorts")
    else:
        _same(base, _oracle(("ties", dtype), pred, conf_thres=0.05, iou_thres=0.5, multi_label=True, max_det=300), "nms_head 0 vs oracle")
    took = 0
    for h in HEADS:
        for sign in (1, -1):
            hv = (_default_head() if h is None else h) * sign
            got, r2 = _run(tune, p, hv, 0.05, 0.5, 300)
            _same(got, base, f"{dtype} nms_head {hv} vs nms_head 0")
            took += r2
    assert took > 0, "no head sent any image to round 2"


# ------------------------------------------------------------------------------------------------ one segment: agnostic, a box beyond max_wh / 2
@pytest.mark.parametrize("agnostic", [False, True])
def test_single_segment_images_beside_partitioned_ones(dev, tune, agnostic):
    """Image 1 holds 40 boxes of 30000 px, two per class, around one centre.  They exceed max_wh / 2, so the image is ONE segment (the emit pass's per-image
    maximum, reduced over its 64 slots): the class offset of 7680 px leaves the boxes of neighbouring classes overlapping by IoU 0.38 > 0.3, and the box of class c
    suppresses those of class c + 1.  A run that partitioned image 1 by class would keep one per class: 20.  Images 0 and 2 are partitioned by class."""
    pred = yo.synth_predictions(bs=3, n_rows=3000, nc=20, seed=9, dtype=torch.float32, hits=0.2)
    i = torch.arange(40)
    pred[1, :40, 0] = 320.0 + i
    pred[1, :40, 1] = 320.0
    pred[1, :40, 2:4] = 30000.0
    pred[1, :40, 4] = 1.0
    pred[1, :40, 5:] = 0.0
    pred[1, i, 5 + i % 20] = 0.95 - i * 0.005
    pred = pred.half()
    want = _oracle(("segment", agnostic), pred, conf_thres=0.05, iou_thres=0.3, multi_label=True, agnostic=agnostic, max_det=300)
    big = int((want[1][:, 2] - want[1][:, 0] > 20000).sum())
    assert big == 1 if agnostic else 1 < big < 20, big
    p = pred.to(dev)
    for h in [0] + HEADS:
        for sign in (1, -1):
            hv = (_default_head() if h is None else h) * sign
            got, _ = _run(tune, p, hv, 0.05, 0.3, 300, agnostic=agnostic)
            _same(got, want, f"agnostic {agnostic} nms_head {hv} vs oracle")


# ------------------------------------------------------------------------------------------------ max_nms against the head
@pytest.mark.parametrize("max_nms", [100, 1000, 30000])
def test_max_nms_below_inside_and_above_the_range(dev, tune, max_nms):
    pred = yo.synth_predictions(bs=2, n_rows=4000, nc=20, seed=7, hits=0.5)
    assert min(_candidates(pred, 0.05)) > 1000   # max_nms = 100 < head = 128 < 1000 < candidates < 30000
    p = pred.to(dev)
    base, _ = _run(tune, p, 0, 0.05, 0.5, 300, max_nms=max_nms)
    for hv in (128, -128, None):
        got, r2 = _run(tune, p, hv, 0.05, 0.5, 300, max_nms=max_nms)
        _same(got, base, f"max_nms {max_nms} nms_head {hv} vs nms_head 0")
        if hv == -128:   # 128 ranks cannot hold 300 kept boxes: round 2, unless max_nms cut the range below the head
            assert r2 == (0 if max_nms <= 128 else 2), r2


# ------------------------------------------------------------------------------------------------ two class passes
def test_more_than_512_classes(dev, tune):
    g = torch.Generator().manual_seed(77)
    pred = torch.rand(2, 1500, 5 + 600, generator=g)
    pred[..., :2] *= 600
    pred[..., 2:4] = pred[..., 2:4] * 60 + 4
    pred[..., 5:] *= (torch.rand(2, 1500, 600, generator=g) < 0.02)   # ~12 labels per row, classes 0 .. 599
    want = _oracle("nc600", pred, conf_thres=0.05, iou_thres=0.5, multi_label=True, max_det=300)
    p = pred.to(dev)
    took = 0
    for hv in (0, 128, -128):
        got, r2 = _run(tune, p, hv, 0.05, 0.5, 300)
        _same(got, want, f"nc 600 nms_head {hv} vs oracle")
        took += r2
    assert took >= 2


# ------------------------------------------------------------------------------------------------ the capacity retry
def test_capacity_overflow_retry_with_both_rounds(dev, tune):
    from yolov3_amd import ops

    g = torch.Generator().manual_seed(3)
    pred = torch.rand(1, 2000, 5 + 10, generator=g)
    pred[..., :2] *= 600
    pred[..., 2:4] *= 80
    pred[..., 4] = 0.5 + 0.5 * pred[..., 4]
    kw = dict(conf_thres=0.001, iou_thres=0.6, max_det=300)
    assert _candidates(pred, 0.001)[0] > 16384   # more than the default capacity of one image: the first call overflows, nms_raw sizes the second by the count
    want = _oracle("overflow", pred, multi_label=True, **kw)
    p = pred.to(dev)
    for hv in (0, 128, -128):
        got, r2 = _run(tune, p, hv, 0.001, 0.6, 300)
        assert ops.nms_raw.last_candidates > 16384
        _same(got, want, f"overflow nms_head {hv} vs oracle")
        if hv == -128:
            assert r2 == 1
