"""GPU tests of the rect train-mode dataset (DeviceRectTrainDataset, the _hw exports of csrc/augment.hip) against tests/golden/augment_rect.pt: the batches the
unmodified reference's LoadImagesAndLabels(augment=True, rect=True, stride=16, pad=0.0) produces for the same cached images from the same seeds
(tests/golden/make_augment_rect_golden.py).  Images must be equal byte for byte, targets bit for bit, paths and shapes equal; no tolerance anywhere.  Case `rect_exact`
rests on the reference alone; the other cases also on the sampler and colour statements of tests/augment_cases.py.
Shapes: batches of 4 at (48, 64), (64, 64) and (64, 48) -- three or four blocks per item -- and, called directly, (16, 48) (768 pixels: one partial block), (48, 80)
(3 840 pixels: the last block partial), (64, 48) and (48, 64): the smallest at which a swapped axis, a wrong row divisor or a wrong tail can show."""
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
import augment_rect_cases as arc  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def gold(golden_dir):
    return torch.load(golden_dir / "augment_rect.pt", weights_only=True)   # data only


@pytest.fixture(scope="module")
def data():
    images, labels, hw, hw0, paths = arc.sorted_set()
    return SimpleNamespace(images=images, labels=labels, hw=hw, hw0=hw0, paths=paths, file_images=ac.make_images(), file_labels=ac.make_labels())


@pytest.fixture(scope="module")
def holder(data, dev):
    """the twelve images in file order in an arena: what the direct calls read (its own batch layout is not used)"""
    from yolov3_amd import DeviceDataset

    return DeviceDataset(data.file_images, data.file_labels, img_size=64, batch_size=4, rect=False, device=dev)


@pytest.fixture(autouse=True)
def _generators_left_alone():
    state = random.getstate(), np.random.get_state()
    yield
    random.setstate(state[0])
    np.random.set_state(state[1])


def _build(data, case, dev):
    """from the images in FILE order: the set sorts them itself"""
    from yolov3_amd import DeviceRectTrainDataset

    c = arc.CASES[case]
    return DeviceRectTrainDataset(data.file_images, data.file_labels, c["hyp"], img_size=arc.IMG_SIZE, batch_size=arc.BATCH, stride=arc.STRIDE, shapes0=ac.hw0(), paths=ac.paths(),
                                  device=dev, dtype=getattr(torch, c["dtype"]))


def _seed(case):
    random.seed(arc.CASES[case]["seed"])
    np.random.seed(arc.CASES[case]["seed"])


def _same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    return a.shape == b.shape and a.dtype == b.dtype == torch.float32 and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _want_images(gold, case, k):
    u8 = arc.expected_images(gold, case, k)
    dtype = getattr(torch, arc.CASES[case]["dtype"])
    return u8 if dtype == torch.uint8 else u8.to(dtype) / 255   # x / 255 rounded once: what `im.to(dtype) / 255` gives


def _epoch(ds, case):
    _seed(case)
    return [(im.cpu(), targets.cpu(), paths, shapes) for im, targets, paths, shapes in ds]


def _assert_epoch(got, gold, case):
    g = gold["cases"][case]
    assert len(got) == len(g["batches"]) == 3
    for k, ((im, targets, paths, shapes), want) in enumerate(zip(got, g["batches"])):
        w = _want_images(gold, case, k)
        assert im.dtype == w.dtype and im.shape == w.shape == (4, 3, *arc.BATCH_SHAPES[k])
        bad = (im != w).nonzero()
        assert torch.equal(im, w), f"{case}: images of batch {k}: {len(bad)} elements differ, first {bad[:4].tolist()}: {im[tuple(bad[0])].item()} != {w[tuple(bad[0])].item()}"
        assert _same_bits(targets, want["targets"]), f"{case}: targets of batch {k}\n{targets}\n{want['targets']}"
        assert isinstance(paths, tuple) and list(paths) == want["paths"] and isinstance(shapes, tuple) and shapes == want["shapes"]


@pytest.mark.parametrize("case", list(arc.CASES))
def test_every_batch_is_the_reference_loaders(data, gold, case, dev):
    ds = _build(data, case, dev)
    assert len(ds) == 3 and ds.rect and [tuple(int(v) for v in s) for s in ds.batch_shapes] == arc.BATCH_SHAPES and ds.order.tolist() == arc.file_index() and ds.paths == data.paths
    im, targets, _, _ = ds.get_batch(0, items=ds.draw_batch(0))
    assert im.device == dev == targets.device and im.is_contiguous() and im.dtype == getattr(torch, arc.CASES[case]["dtype"])
    first = _epoch(ds, case)
    _assert_epoch(first, gold, case)
    after = random.random(), float(np.random.random())
    again = _epoch(ds, case)   # the same epoch from the same seeds: identical bytes, and the generators end where they ended
    assert all(torch.equal(a[0], b[0]) and _same_bits(a[1], b[1]) and a[2:] == b[2:] for a, b in zip(first, again)) and (random.random(), float(np.random.random())) == after
    with pytest.raises(ValueError, match="rect=True set keeps its aspect-ratio order"):
        ds.set_indices(list(range(12)))


def test_from_dataset_on_a_reference_dataset(data, gold, dev):
    from yolov3_amd import DeviceRectTrainDataset

    for case in ("rect_low", "rect_wild", "rect_low_f16"):
        c, g = arc.CASES[case], gold["cases"][case]
        ref = SimpleNamespace(ims=data.images, im_hw0=data.hw0, im_hw=data.hw, labels=[lb.copy() for lb in data.labels], segments=[[] for _ in data.labels], im_files=data.paths,
                              rect=True, img_size=arc.IMG_SIZE, stride=arc.STRIDE, augment=True, mosaic=False, hyp=dict(c["hyp"]), n=12, indices=range(12), pad=0.0,
                              batch=np.array(g["batch"]), batch_shapes=np.array(g["batch_shapes"]))
        ds = DeviceRectTrainDataset.from_dataset(ref, batch_size=arc.BATCH, device=dev, dtype=getattr(torch, c["dtype"]))
        assert ds.order.tolist() == list(range(12))   # the order the dataset is already in is adopted
        _assert_epoch(_epoch(ds, case), gold, case)


def _hand_item(i, hw, H, W, M, scale, luts):
    """image i centred on an H x W canvas as letterbox centres it (cropped where it is larger: negative halves), both flips on"""
    from yolov3_amd import augment

    h, w = hw[i]
    dw, dh = (W - w) / 2, (H - h) / 2
    top, left = round(dh - 0.1), round(dw - 0.1)
    x1a, y1a, x2a, y2a = max(left, 0), max(top, 0), min(left + w, W), min(top + h, H)
    rect = (x1a, y1a, x2a, y2a, x1a - left, y1a - top, x2a - left, y2a - top)
    return augment.Item(i, [augment.Mosaic([i], [rect], M, scale, W, [(dw, dh)], None, H)], None, luts, True, True, False)


@pytest.mark.parametrize("shape", [(16, 48), (48, 80), (64, 48), (48, 64)])
def test_the_hw_exports_on_hand_made_records(data, holder, dev, shape):
    from yolov3_amd import augment, ops

    H, W = shape
    hyp = arc.CASES["rect_wild"]["hyp"]
    random.seed(1000 * H + W)
    x = np.arange(256)
    items = []
    for slot, i in enumerate((6, 10, 4, 2)):   # 16x64, 30x64, 51x64, 64x64: wider or higher than some of the shapes, so the crop and negative halves occur
        M, scale = augment.draw_perspective(hyp, (H, W), 0)
        luts = np.stack([(x * (1 + 0.01 * slot)) % 180, np.clip(x * (0.6 + 0.2 * slot), 0, 255), np.clip(x * (1.3 - 0.2 * slot), 0, 255)]).astype(np.uint8)
        items.append(_hand_item(i, ac.hw(), H, W, M, scale, luts if slot else None))
    rec = torch.from_numpy(augment.pack_items(items).view(np.uint8).copy()).to(dev)
    guard = torch.full((6, 3, H, W), 77, dtype=torch.uint8, device=dev)   # a slice of a larger buffer: the images before and behind keep their bytes
    im = ops.augment_batch_hw(holder._arena, holder._records, holder.n, rec, 4, H, W, torch.uint8, out=guard[1:-1])
    want = np.stack([arc.item_image(it, data.file_images, H, W) for it in items])
    assert im.shape == (4, 3, H, W) and np.array_equal(im.cpu().numpy(), want), f"{shape}: {(im.cpu().numpy() != want).sum()} bytes differ"
    assert (guard[0] == 77).all() and (guard[-1] == 77).all()
    f32 = ops.augment_batch_hw(holder._arena, holder._records, holder.n, rec, 4, H, W, torch.float32)
    assert torch.equal(f32.cpu(), torch.from_numpy(want).float() / 255)
    upper = sum(len(data.file_labels[it.index]) for it in items)
    targets, offsets = ops.augment_targets_hw(holder._labels, holder._label_offsets, holder._records, holder.n, rec, 4, H, W, upper)
    want_t = torch.from_numpy(arc.batch_targets(items, data.file_labels, ac.hw(), H, W))
    nl = int(offsets.cpu()[-1])
    assert nl == len(want_t) > 0 and offsets.cpu().tolist() == [0] + torch.cumsum(torch.bincount(want_t[:, 0].long(), minlength=4), 0).tolist()
    assert _same_bits(targets[:nl].cpu(), want_t), f"{shape}\n{targets[:nl].cpu()}\n{want_t}"


def test_the_square_exports_and_the_hw_exports_agree_on_a_square_batch(data, holder, golden_dir, dev):
    """one `low` batch of DeviceTrainDataset's (four mosaics, mixup off): identical bytes through y3_augment_batch / _targets and through the _hw exports with H = W = 64"""
    from yolov3_amd import augment, ops

    c = ac.CASES["low"]
    random.seed(c["seed"])
    np.random.seed(c["seed"])
    items = [augment.draw_item(i, ac.hw(), c["hyp"], ac.IMG_SIZE, range(12), 12, True) for i in range(4)]
    assert all(it.mosaic for it in items)
    rec = torch.from_numpy(augment.pack_items(items).view(np.uint8).copy()).to(dev)
    upper = sum(len(data.file_labels[j]) for it in items for mo in it.mosaics for j in mo.indices)
    want = torch.load(golden_dir / "augment.pt", weights_only=True)["cases"]["low"]["batches"][0]
    for dtype in (torch.uint8, torch.float16):
        a = ops.augment_batch(holder._arena, holder._records, holder.n, rec, 4, 64, dtype)
        b = ops.augment_batch_hw(holder._arena, holder._records, holder.n, rec, 4, 64, 64, dtype)
        assert torch.equal(a, b) and (dtype != torch.uint8 or torch.equal(a.cpu(), want["im"]))
    ta, oa = ops.augment_targets(holder._labels, holder._label_offsets, holder._records, holder.n, rec, 4, 64, upper)
    tb, ob = ops.augment_targets_hw(holder._labels, holder._label_offsets, holder._records, holder.n, rec, 4, 64, 64, upper)
    nl = int(oa.cpu()[-1])
    assert torch.equal(oa, ob) and _same_bits(ta[:nl].cpu(), tb[:nl].cpu()) and _same_bits(ta[:nl].cpu(), want["targets"])


def test_rect_records_that_point_outside_read_nothing(data, holder, dev):
    """the kernel's own bound on a 64 wide, 48 high canvas: tiles whose image, rectangle or offsets do not fit are cut down to the image AND the canvas, or dropped"""
    from yolov3_amd import augment, ops

    M = np.array([[1.0, 0, 0], [0, 1, -10], [0, 0, 1]])   # output row y shows canvas row y + 10: rows 48 .. 57 of the canvas do not exist, though image 0 has them
    whole = (0, 0, 128, 128, 0, 0, 128, 128)   # claims far more than the canvas for a 64 x 48 image at (0, 0)
    items = [augment.Item(0, [augment.Mosaic([0, 12, -1, 0], [whole, whole, whole, (50, 40, 64, 48, 0, 0, 14, 8)], M, 1.0, 64, [(0, 0)] * 4, None, 48)], None, None, False, False,
                          False)]
    rec = augment.pack_items(items)
    rec["mosaics"][0, 0]["tiles"][3]["padw"], rec["mosaics"][0, 0]["tiles"][3]["padh"] = -5000, -5000   # the source pixel of that tile lies far outside its image
    dev_rec = torch.from_numpy(rec.view(np.uint8).copy()).to(dev)
    im = ops.augment_batch_hw(holder._arena, holder._records, holder.n, dev_rec, 1, 48, 64).cpu()
    canvas = np.full((48, 64, 3), 114, dtype=np.uint8)
    canvas[:48, :48] = data.file_images[0][:48]
    want = ac.warp_affine_u8(canvas, M[:2], (64, 48))
    assert (want[38:] == 114).all() and np.array_equal(im[0].numpy(), want.transpose(2, 0, 1)[::-1])
    targets, offsets = ops.augment_targets_hw(holder._labels, holder._label_offsets, holder._records, holder.n, dev_rec, 1, 48, 64, 64)
    assert offsets.cpu()[0] == 0 and 0 <= int(offsets.cpu()[1]) <= 2 * len(data.file_labels[0])


def test_a_yielded_rect_batch_feeds_the_train_step(dev):
    """one ComputeLoss forward / backward of yolov3-tiny at width 0.25 on a 128 x 64 batch as the set yields it, and on the same tensors passed in directly"""
    import yaml

    from yolov3_amd import ComputeLoss, DetectionModel, DeviceRectTrainDataset

    rs = np.random.RandomState(5)
    images = [rs.randint(0, 256, (128, w, 3), dtype=np.uint8) for w in (64, 57, 60, 64)]
    labels = [np.concatenate([rs.randint(0, 80, (3, 1)), rs.uniform(0.3, 0.7, (3, 2)), rs.uniform(0.2, 0.5, (3, 2))], 1).astype(np.float32) for _ in images]
    d = yaml.safe_load(open(ROOT / "yolov3_amd" / "cfg" / "yolov3-tiny.yaml"))
    d["width_multiple"] = 0.25
    torch.manual_seed(3)
    m = DetectionModel(d, ch=3, nc=80).to(dev).float().train()
    m.hyp = dict(box=0.05, cls=0.5, cls_pw=1.0, obj=1.0, obj_pw=1.0, anchor_t=4.0, fl_gamma=0.0, label_smoothing=0.0)
    crit = ComputeLoss(m)
    ds = DeviceRectTrainDataset(images, labels, arc.CASES["rect_low"]["hyp"], img_size=128, batch_size=4, stride=32, device=dev, dtype=torch.float32)
    assert len(ds) == 1 and ds.batch_shapes.tolist() == [[128, 64]]
    _seed("rect_low")
    im, targets, paths, shapes = next(iter(ds))
    assert im.shape == (4, 3, 128, 64) and im.dtype == torch.float32 and 0 <= float(im.min()) and float(im.max()) <= 1 and len(targets) > 0
    assert all(s is not None and s[0] == (128, w) for s, w in zip(shapes, (64, 64, 60, 57)))   # the aspect-ratio order: h / w ascending (the sort is not stable)
    loss, parts = crit(m(im), targets)
    loss.backward()
    assert torch.isfinite(loss).all() and torch.isfinite(parts).all() and float(loss.detach()) > 0
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in m.parameters() if p.requires_grad)
    direct, _ = crit(m(im.clone()), targets.clone())
    assert torch.equal(direct.detach(), loss.detach())
