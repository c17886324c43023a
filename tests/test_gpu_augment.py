"""GPU tests of the train-mode dataset (csrc/augment.hip through yolov3_amd/augment.py) against tests/golden/augment.pt: the batches the unmodified reference's
LoadImagesAndLabels.__getitem__ (augment=True: load_mosaic, random_perspective, mixup, augment_hsv, the flips) and collate_fn produce for the same cached images from
the same seeds (tests/golden/make_augment_golden.py).  Images must be equal byte for byte, targets bit for bit, paths and shapes equal; no tolerance anywhere.  Case
`exact` rests on the reference alone; the other cases also on the sampler and colour statements of tests/augment_cases.py.
Shapes: 12 images with a long side of 64, batches of 4, 64 px: four blocks per item, odd source widths, every branch of the two kernels."""
import random
import sys
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests"))

import augment_cases as ac  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def gold(golden_dir):
    return torch.load(golden_dir / "augment.pt", weights_only=True)   # data only


@pytest.fixture(scope="module")
def data():
    return SimpleNamespace(images=ac.make_images(), labels=ac.make_labels())


@pytest.fixture(autouse=True)
def _generators_left_alone():
    state = random.getstate(), np.random.get_state()
    yield
    random.setstate(state[0])
    np.random.set_state(state[1])


def _build(data, case, dev):
    from yolov3_amd import DeviceTrainDataset

    c = ac.CASES[case]
    ds = DeviceTrainDataset(data.images, data.labels, c["hyp"], img_size=ac.IMG_SIZE, batch_size=ac.BATCH, stride=ac.STRIDE, shapes0=ac.hw0(), paths=ac.paths(), device=dev,
                            dtype=getattr(torch, c["dtype"]))
    if c["indices"] is not None:
        ds.set_indices(c["indices"])
    return ds


def _seed(case):
    random.seed(ac.CASES[case]["seed"])
    np.random.seed(ac.CASES[case]["seed"])


def _same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    return a.shape == b.shape and a.dtype == b.dtype == torch.float32 and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _want_images(gold, case, k):
    u8 = ac.expected_images(gold, case, k)
    dtype = getattr(torch, ac.CASES[case]["dtype"])
    return u8 if dtype == torch.uint8 else u8.to(dtype) / 255   # the 256-entry quotient table: what `im.to(dtype) / 255` gives


def _epoch(ds, case):
    _seed(case)
    return [(im.cpu(), targets.cpu(), paths, shapes) for im, targets, paths, shapes in ds]


def _assert_epoch(got, gold, case, dev=None):
    g = gold["cases"][case]
    assert len(got) == len(g["batches"])
    for k, ((im, targets, paths, shapes), want) in enumerate(zip(got, g["batches"])):
        w = _want_images(gold, case, k)
        assert im.dtype == w.dtype and im.shape == w.shape
        bad = (im != w).nonzero()
        assert torch.equal(im, w), f"{case}: images of batch {k}: {len(bad)} elements differ, first {bad[:4].tolist()}: {im[tuple(bad[0])].item()} != {w[tuple(bad[0])].item()}"
        assert _same_bits(targets, want["targets"]), f"{case}: targets of batch {k}\n{targets}\n{want['targets']}"
        assert isinstance(paths, tuple) and list(paths) == want["paths"] and isinstance(shapes, tuple) and shapes == want["shapes"]


@pytest.mark.parametrize("case", list(ac.CASES))
def test_every_batch_is_the_reference_loaders(data, gold, case, dev):
    ds = _build(data, case, dev)
    im, targets, _, _ = ds.get_batch(0, items=ds.draw_batch(0))
    assert im.device == dev == targets.device and im.is_contiguous() and im.dtype == getattr(torch, ac.CASES[case]["dtype"])
    first = _epoch(ds, case)
    _assert_epoch(first, gold, case)
    after = random.random(), float(np.random.random())
    again = _epoch(ds, case)   # the same epoch from the same seeds: identical bytes, and the generators end where they ended
    assert all(torch.equal(a[0], b[0]) and _same_bits(a[1], b[1]) and a[2:] == b[2:] for a, b in zip(first, again)) and (random.random(), float(np.random.random())) == after


def test_set_indices_with_a_permutation_and_a_repeating_draw(data, gold, dev):
    """`wild` sets indices: a permutation of the twelve images followed by a draw that repeats one (the pool of load_mosaic's random.choices as well)"""
    from yolov3_amd import DeviceTrainDataset

    c = ac.CASES["wild"]
    assert sorted(c["indices"][:12]) == list(range(12)) != c["indices"][:12] and c["indices"][12:] == [5, 5, 2, 5]
    ds = DeviceTrainDataset(data.images, data.labels, c["hyp"], img_size=ac.IMG_SIZE, batch_size=ac.BATCH, stride=ac.STRIDE, shapes0=ac.hw0(), paths=ac.paths(), device=dev)
    assert len(ds) == 3
    ds.set_indices(np.array(c["indices"]))
    assert len(ds) == 4 and ds.batch_images(3) == [5, 5, 2, 5]
    _assert_epoch(_epoch(ds, "wild"), gold, "wild")
    ds.set_indices(None)
    assert len(ds) == 3


def test_from_dataset_on_a_reference_dataset(data, gold, dev):
    from yolov3_amd import DeviceTrainDataset

    for case in ("low", "wild", "single", "low_f16"):
        c = ac.CASES[case]
        labels = [lb.copy() for lb in data.labels]
        ref = SimpleNamespace(ims=data.images, im_hw0=ac.hw0(), im_hw=ac.hw(), labels=labels, segments=[[] for _ in labels], im_files=ac.paths(), rect=False, img_size=ac.IMG_SIZE,
                              stride=ac.STRIDE, augment=True, mosaic=True, hyp=dict(c["hyp"]), n=12, indices=c["indices"] if c["indices"] is not None else range(12))
        ds = DeviceTrainDataset.from_dataset(ref, batch_size=ac.BATCH, device=dev, dtype=getattr(torch, c["dtype"]))
        _assert_epoch(_epoch(ds, case), gold, case)


def test_offsets_and_the_upper_bound_of_the_targets(data, gold, dev):
    from yolov3_amd import augment, ops

    ds = _build(data, "exact", dev)
    _seed("exact")
    for k, want in enumerate(gold["cases"]["exact"]["batches"]):
        items = ds.draw_batch(k)
        rec = torch.from_numpy(augment.pack_items(items).view(np.uint8).copy()).to(dev)
        upper = sum(len(data.labels[j]) for it in items for mo in it.mosaics for j in mo.indices)
        targets, offsets = ops.augment_targets(ds._labels, ds._label_offsets, ds._records, ds.n, rec, len(items), ac.IMG_SIZE, upper)
        counts = torch.bincount(want["targets"][:, 0].long(), minlength=len(items))
        assert offsets.dtype == torch.int64 and offsets.cpu().tolist() == [0] + torch.cumsum(counts, 0).tolist() and upper >= len(want["targets"]) and targets.shape == (upper, 6)
        assert _same_bits(targets[: len(want["targets"])].cpu(), want["targets"])
        guard = torch.full((len(items) + 2, 3, 64, 64), 77, dtype=torch.uint8, device=dev)   # a slice of a larger buffer: the images before and behind keep their bytes
        ops.augment_batch(ds._arena, ds._records, ds.n, rec, len(items), ac.IMG_SIZE, torch.uint8, out=guard[1:-1])
        assert torch.equal(guard[1:-1].cpu(), want["im"]) and (guard[0] == 77).all() and (guard[-1] == 77).all()


def test_records_that_point_outside_read_nothing(data, dev):
    """the kernel's own bound: tiles whose image, rectangle or offsets do not fit are cut down or dropped, never read"""
    from yolov3_amd import augment, ops

    ds = _build(data, "exact", dev)
    M = np.array([[1.0, 0, -32], [0, 1, -32], [0, 0, 1]])
    whole = (0, 0, 128, 128, 0, 0, 128, 128)   # claims the whole canvas for a 64 x 48 image at (0, 0)
    items = [augment.Item(0, [augment.Mosaic([0, 12, -1, 0], [whole, whole, whole, (100, 100, 128, 128, 0, 0, 28, 28)], M, 1.0, 128, [(0, 0)] * 3 + [(-5000, -5000)])], None, None,
                          False, False, True)]
    rec = augment.pack_items(items)
    rec["mosaics"][0, 0]["tiles"][3]["padw"], rec["mosaics"][0, 0]["tiles"][3]["padh"] = -5000, -5000   # the source pixel of that tile lies far outside its image
    im = ops.augment_batch(ds._arena, ds._records, ds.n, torch.from_numpy(rec.view(np.uint8).copy()).to(dev), 1, 64).cpu()
    want = np.full((128, 128, 3), 114, dtype=np.uint8)
    want[:64, :48] = data.images[0]
    assert np.array_equal(im[0].numpy(), want[32:96, 32:96].transpose(2, 0, 1)[::-1])
    targets, offsets = ops.augment_targets(ds._labels, ds._label_offsets, ds._records, ds.n, torch.from_numpy(rec.view(np.uint8).copy()).to(dev), 1, 64, 64)
    assert offsets.cpu()[0] == 0 and 0 <= int(offsets.cpu()[1]) <= 2 * len(data.labels[0])


def test_a_yielded_batch_feeds_the_train_step(data, dev):
    """one ComputeLoss forward / backward of yolov3-tiny at 64 x 64 on a batch as the set yields it: the 4-tuple feeds the train path unchanged"""
    from yolov3_amd import ComputeLoss, DetectionModel, DeviceTrainDataset

    torch.manual_seed(3)
    m = DetectionModel("yolov3-tiny.yaml", nc=80).to(dev).float().train()
    m.hyp = dict(box=0.05, cls=0.5, cls_pw=1.0, obj=1.0, obj_pw=1.0, anchor_t=4.0, fl_gamma=0.0, label_smoothing=0.0)
    crit = ComputeLoss(m)
    ds = DeviceTrainDataset(data.images, data.labels, ac.CASES["low"]["hyp"], img_size=ac.IMG_SIZE, batch_size=ac.BATCH, stride=ac.STRIDE, paths=ac.paths(), device=dev,
                            dtype=torch.float32)
    _seed("low")
    im, targets, paths, shapes = next(iter(ds))
    assert im.shape == (4, 3, 64, 64) and im.dtype == torch.float32 and 0 <= float(im.min()) and float(im.max()) <= 1 and len(targets) > 0 and shapes == (None,) * 4
    loss, parts = crit(m(im), targets)
    loss.backward()
    assert torch.isfinite(loss).all() and torch.isfinite(parts).all() and float(loss.detach()) > 0
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in m.parameters() if p.requires_grad)
