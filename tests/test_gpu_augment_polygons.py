"""GPU tests of polygon labels in the train-mode dataset (y3_augment_polygons, y3_augment_targets_polygons of csrc/augment.hip through yolov3_amd/augment.py) against
tests/golden/augment_polygons.pt: the targets the unmodified reference's loader produces over polygon label files from the same seeds, the fp64 polygon boxes and the
path word per mosaic of the statement of tests/augment_polygon_cases.py (asserted equal to the reference by the generator).  Targets bit for bit, boxes bit for bit in
fp64, images equal to those of the same set without its polygons; no tolerance anywhere.
Shapes: 12 images with a long side of 64, batches of 4: up to 21 label rows per mosaic (more rows than the 4 waves of a block), polygons of 1 to 1203 vertices."""
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
import augment_polygon_cases as apc  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def gold(golden_dir):
    return torch.load(golden_dir / "augment_polygons.pt", weights_only=True)   # data only


@pytest.fixture(scope="module")
def data():
    labels, segments = apc.make_polygons()
    return SimpleNamespace(images=ac.make_images(), labels=labels, segments=segments)


@pytest.fixture(autouse=True)
def _generators_left_alone():
    state = random.getstate(), np.random.get_state()
    yield
    random.setstate(state[0])
    np.random.set_state(state[1])


def _build(data, case, dev, segments="own", **kw):
    from yolov3_amd import DeviceTrainDataset

    c = apc.CASES[case]
    ds = DeviceTrainDataset(data.images, data.labels, c["hyp"], img_size=ac.IMG_SIZE, batch_size=ac.BATCH, stride=ac.STRIDE, shapes0=ac.hw0(), paths=ac.paths(), device=dev,
                            segments=data.segments if segments == "own" else segments, **kw)
    if c["indices"] is not None:
        ds.set_indices(c["indices"])
    return ds


def _seed(case):
    random.seed(apc.CASES[case]["seed"])
    np.random.seed(apc.CASES[case]["seed"])


def _bits(a: torch.Tensor) -> torch.Tensor:
    return a.contiguous().view(torch.int32 if a.dtype == torch.float32 else torch.int64)


def _assert_workspace(ds, want, upper, what):
    boxes, inside, words = (t.cpu() for t in ds.polygons)
    assert boxes.shape == (upper, 4) and boxes.dtype == torch.float64 and inside.shape == (upper,) and words.shape == (len(want["words"]), 2)
    assert torch.equal(words, want["words"]), f"{what}: path words\n{words}\n{want['words']}"
    w = want["written"]
    assert torch.equal(_bits(boxes[w]), _bits(want["boxes"][w])), f"{what}: polygon boxes\n{boxes[w]}\n{want['boxes'][w]}"
    assert torch.equal(inside[w], want["inside"][w])


@pytest.mark.parametrize("case", list(apc.CASES))
def test_every_batch_is_the_reference_loaders(data, gold, case, dev):
    ds, plain = _build(data, case, dev), _build(data, case, dev, segments=None)
    assert ds._vertices.shape == (sum(len(p) for sg in data.segments for p in sg), 2) and ds._vertex_offsets.shape == (sum(ac.LABEL_COUNTS) + 1,) and plain._vertices is None
    g = gold["cases"][case]
    assert len(ds) == len(g["batches"])
    _seed(case)
    got = []
    for k, want in enumerate(g["batches"]):
        items = ds.draw_batch(k)
        im, targets, paths, shapes = ds.get_batch(k, items=items)
        got.append((im.cpu(), items))
        assert targets.device == dev and targets.dtype == torch.float32 and targets.shape == want["targets"].shape, f"{case}: batch {k}: {targets.shape[0]} targets, {want['targets'].shape[0]} wanted"
        assert torch.equal(_bits(targets.cpu()), _bits(want["targets"])), f"{case}: targets of batch {k}\n{targets.cpu()}\n{want['targets']}"
        assert list(paths) == want["paths"]
        _assert_workspace(ds, want, sum(len(data.labels[j]) for it in items for mo in it.mosaics for j in mo.indices), f"{case}: batch {k}")
        assert torch.equal(ds.polygons[2].cpu() == apc.PATH_NONZERO, want["reference_resampled"])   # the path the reference took
    assert (random.random(), float(np.random.random())) == (g["batches"][-1]["next_random"], g["batches"][-1]["next_np_random"])   # polygons draw no random numbers
    for k, (im, items) in enumerate(got):   # the images are those of the same set without its polygons
        assert torch.equal(im, plain.get_batch(k, items=items)[0].cpu()), f"{case}: polygons changed the images of batch {k}"


def test_offsets_and_the_ops_directly(data, gold, dev):
    from yolov3_amd import augment, ops

    ds = _build(data, "wild", dev)
    _seed("wild")
    for k, want in enumerate(gold["cases"]["wild"]["batches"]):
        items = ds.draw_batch(k)
        rec = torch.from_numpy(augment.pack_items(items).view(np.uint8).copy()).to(dev)
        upper = sum(len(data.labels[j]) for it in items for mo in it.mosaics for j in mo.indices)
        ws = ops.augment_polygons(ds._vertices, ds._vertex_offsets, ds._label_offsets, ds._records, ds.n, rec, len(items), ac.IMG_SIZE, upper)
        targets, offsets = ops.augment_targets_polygons(ds._labels, ds._label_offsets, ds._records, ds.n, rec, len(items), ac.IMG_SIZE, upper, *ws)
        counts = torch.bincount(want["targets"][:, 0].long(), minlength=len(items))
        assert offsets.dtype == torch.int64 and offsets.cpu().tolist() == [0] + torch.cumsum(counts, 0).tolist() and targets.shape == (upper, 6) and upper >= len(want["targets"])
        assert torch.equal(_bits(targets[: len(want["targets"])].cpu()), _bits(want["targets"]))
        # the box form on the same records is untouched by the polygon tables: what a box-only set of these labels yields
        box_targets, box_offsets = ops.augment_targets(ds._labels, ds._label_offsets, ds._records, ds.n, rec, len(items), ac.IMG_SIZE, upper)
        st = [apc.polygon_labels(it, data.labels, [[] for _ in data.labels], ac.hw(), ac.IMG_SIZE)["targets"] for it in items]
        assert int(box_offsets.cpu()[-1]) == sum(len(t) for t in st)
        assert np.array_equal(box_targets[: int(box_offsets.cpu()[-1]), 1:].cpu().numpy().view(np.int32), np.concatenate(st, 0).view(np.int32))


def test_polygons_that_all_clip_to_zero_fall_back_to_the_box_path(dev):
    """Every polygon of every mosaic lies beyond the canvas origin and clips to all zeros while the label boxes do not: any(x.any()) is False, the box path with
    area_thr 0.10.  Not reachable from the reference's parser (there the box is derived from the polygon): the expectations are the statement's alone."""
    from yolov3_amd import DeviceTrainDataset

    images, labels, segments, hw = apc.zero_polygon_set()
    hyp = dict(apc.CASES["low"]["hyp"], mixup=0.5)
    ds = DeviceTrainDataset(images, labels, hyp, img_size=ac.IMG_SIZE, batch_size=4, stride=ac.STRIDE, paths=ac.paths()[:4], device=dev, segments=segments)
    plain = DeviceTrainDataset(images, labels, hyp, img_size=ac.IMG_SIZE, batch_size=4, stride=ac.STRIDE, paths=ac.paths()[:4], device=dev)
    random.seed(3)
    np.random.seed(3)
    items = ds.draw_batch(0)
    assert any(len(it.mosaics) == 2 for it in items)
    st = apc.batch_statement(items, labels, segments, hw, ac.IMG_SIZE)
    # every word is 0: nothing is non-zero and no row lacks a polygon
    assert not st["words"].any() and len(st["targets"]) > 0
    _, targets, _, _ = ds.get_batch(0, items=items)
    assert torch.equal(_bits(targets.cpu()), _bits(torch.from_numpy(st["targets"])))
    assert torch.equal(ds.polygons[2].cpu(), torch.from_numpy(st["words"]))
    assert torch.equal(_bits(targets.cpu()), _bits(plain.get_batch(0, items=items)[1].cpu()))   # and what the set without its polygons yields


def test_set_indices_with_a_repeating_draw(data, gold, dev):
    """`wild` ends in the draw [5, 5, 2, 5]: the same image in several tiles of a batch, at different pads, reads the same vertices"""
    c = apc.CASES["wild"]
    assert c["indices"][12:] == [5, 5, 2, 5]
    ds = _build(data, "wild", dev)
    assert len(ds) == 4 and ds.batch_images(3) == [5, 5, 2, 5]
    _seed("wild")
    for k, want in enumerate(gold["cases"]["wild"]["batches"]):
        items = ds.draw_batch(k)
        targets = ds.get_batch(k, items=items)[1]
        if k == 3:
            tiles = [(j, pad) for it in items for mo in it.mosaics for j, pad in zip(mo.indices, mo.pad)]
            assert any(len({pad for j, pad in tiles if j == i}) > 1 for i in range(12))   # one image, two pads
            assert torch.equal(_bits(targets.cpu()), _bits(want["targets"]))
    ds.set_indices(None)
    assert len(ds) == 3


def test_from_dataset_and_a_yielded_batch_feeds_the_train_step(data, dev):
    from yolov3_amd import ComputeLoss, DetectionModel, DeviceTrainDataset

    ref = SimpleNamespace(ims=data.images, im_hw0=ac.hw0(), im_hw=ac.hw(), labels=data.labels, segments=data.segments, im_files=ac.paths(), rect=False, img_size=ac.IMG_SIZE,
                          stride=ac.STRIDE, augment=True, mosaic=True, hyp=dict(apc.CASES["low"]["hyp"]), n=12, indices=range(12))
    ds = DeviceTrainDataset.from_dataset(ref, batch_size=ac.BATCH, device=dev, dtype=torch.float32)
    assert ds._vertices is not None
    torch.manual_seed(3)
    m = DetectionModel("yolov3-tiny.yaml", nc=80).to(dev).float().train()
    m.hyp = dict(box=0.05, cls=0.5, cls_pw=1.0, obj=1.0, obj_pw=1.0, anchor_t=4.0, fl_gamma=0.0, label_smoothing=0.0)
    crit = ComputeLoss(m)
    _seed("low")
    im, targets, paths, shapes = next(iter(ds))
    assert im.shape == (4, 3, 64, 64) and im.dtype == torch.float32 and len(targets) > 0 and shapes == (None,) * 4
    loss, parts = crit(m(im), targets)
    loss.backward()
    assert torch.isfinite(loss).all() and torch.isfinite(parts).all() and float(loss.detach()) > 0
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in m.parameters() if p.requires_grad)
