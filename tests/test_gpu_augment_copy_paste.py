"""GPU tests of copy-paste in the train-mode dataset (y3_augment_copy_paste_select, y3_augment_copy_paste_raster, y3_augment_batch_paste, y3_augment_polygons_paste,
y3_augment_targets_paste of csrc/augment.hip through yolov3_amd/augment.py) against tests/golden/augment_copy_paste.pt -- what the unmodified reference's loader
produces with copy_paste 0.1, 0.5 and 1.0 over the polygon label files, from the same seeds -- and against the NumPy statement of tests/augment_copy_paste_cases.py
(asserted equal to the reference item by item by the generator).  Images, targets, accepted lists and masks bit for bit; no tolerance anywhere.
Shapes: 12 images with a long side of 64 (canvas 128), batches of 4; hand-made sets at canvas 32 and 128 whose mosaics hold twelve polygons (more accepted pastes than a
block has waves), among them polygons of 1024, 1025 and 1203 vertices: on and on either side of the 1024 edges the raster keeps in LDS."""
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
import augment_copy_paste_cases as cpc  # noqa: E402
import augment_polygon_cases as apc  # noqa: E402
import augment_rect_cases as arc  # noqa: E402

pytestmark = pytest.mark.gpu
CASES = cpc.cases()


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def gold(golden_dir):
    return torch.load(golden_dir / "augment_copy_paste.pt", weights_only=True)   # data only


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


def _seed(seed):
    random.seed(seed)
    np.random.seed(seed)


def _build(data, hyp, dev, indices=None, segments="own", **kw):
    from yolov3_amd import DeviceTrainDataset

    ds = DeviceTrainDataset(data.images, data.labels, hyp, img_size=ac.IMG_SIZE, batch_size=ac.BATCH, stride=ac.STRIDE, shapes0=ac.hw0(), paths=ac.paths(), device=dev,
                            segments=data.segments if segments == "own" else segments, **kw)
    if indices is not None:
        ds.set_indices(indices)
    return ds


def _bits(a: torch.Tensor) -> torch.Tensor:
    return a.contiguous().view(torch.int32)


def _assert_pastes(ds, items, st, what):
    """the accepted lists and the masks the device left for the batch (ds.pastes) against the statement's"""
    from yolov3_amd import augment

    if not any(mo.paste for it in items if it.mosaic for mo in it.mosaics):
        assert ds.pastes is None and not any(st["accepted"])
        return
    table, nk, n_masks = augment.pack_paste(items)
    sel_i, sel_f, masks = (t.cpu() for t in ds.pastes)
    assert sel_i.shape == (nk, 4) and sel_f.shape == (nk, 5) and masks.shape[0] == n_masks
    bits = ((masks.unsqueeze(-1) >> torch.arange(32, dtype=torch.int32)) & 1).bool().reshape(n_masks, masks.shape[1], -1).numpy()   # bit x & 31 of word x >> 5
    count = len(items)
    for slot in range(2 * count):
        lo, hi, mi = int(table[slot]), int(table[slot + 1]), int(table[2 * count + 1 + slot])
        got = [(e, int(sel_i[lo + e, 1]), sel_f[lo + e, 1:]) for e in range(hi - lo) if int(sel_i[lo + e, 0])]
        want = st["accepted"][slot]
        assert [(e, j) for e, j, _ in got] == [(e, j) for e, j, _ in want], f"{what}: the accepted candidates of mosaic {slot}"
        assert all(torch.equal(_bits(b), _bits(torch.from_numpy(wb))) for (_, _, b), (_, _, wb) in zip(got, want)), f"{what}: the boxes of mosaic {slot}"
        if mi >= 0:
            assert np.array_equal(bits[mi], st["masks"][slot]), f"{what}: the mask of mosaic {slot} differs in {int((bits[mi] != st['masks'][slot]).sum())} pixels"
        else:
            assert st["masks"][slot] is None


@pytest.mark.parametrize("case", list(CASES))
def test_every_batch_is_the_reference_loaders(data, gold, case, dev):
    c, g = CASES[case], gold["cases"][case]
    ds = _build(data, c["hyp"], dev, c["indices"], copy_paste=True)
    assert len(ds) == len(g["batches"])
    _seed(c["seed"])
    for k, want in enumerate(g["batches"]):
        items = ds.draw_batch(k)
        assert [list(it.mosaics[m].paste) if m < len(it.mosaics) else [] for it in items for m in range(2)] == want["pastes"]
        im, targets, paths, shapes = ds.get_batch(k, items=items)
        assert im.device == dev == targets.device and im.dtype == torch.uint8 and targets.shape == want["targets"].shape, f"{case}: batch {k}: {targets.shape[0]} targets, {want['targets'].shape[0]} wanted"
        assert torch.equal(_bits(targets.cpu()), _bits(want["targets"])), f"{case}: targets of batch {k}\n{targets.cpu()}\n{want['targets']}"
        st = cpc.batch_statement(items, data.images, data.labels, data.segments, ac.hw(), ac.IMG_SIZE)
        assert cpc.crc(st["im"]) == want["im_crc"]   # the statement's image is the reference's
        assert torch.equal(im.cpu(), torch.from_numpy(st["im"])), f"{case}: image of batch {k}: {int((im.cpu() != torch.from_numpy(st['im'])).sum())} bytes differ"
        assert list(paths) == want["paths"] and torch.equal(ds.polygons[2].cpu(), want["words"])
        assert [[(e, j) for e, j, _ in a] for a in st["accepted"]] == [[(e, j) for e, j, _ in a] for a in want["accepted"]]
        _assert_pastes(ds, items, st, f"{case}: batch {k}")
    assert (random.random(), float(np.random.random())) == (g["batches"][-1]["next_random"], g["batches"][-1]["next_np_random"])


@pytest.mark.parametrize("s", [16, 64])
def test_hand_made_polygons_at_canvas_32_and_128(s, dev):
    """concave, self-intersecting, 1203 vertices, horizontal edges, vertices clipped onto 0 and 2 S, one and two vertices; every mirrored box accepted, so a mosaic
    rasterises more polygons than a block has waves.  Not reachable from the reference's parser (the boxes are not those of the polygons): the statement's alone."""
    from yolov3_amd import DeviceTrainDataset

    images, labels, segments, hw = cpc.raster_set(s)
    hyp = dict(apc.CASES["wild"]["hyp"], copy_paste=1.0, mixup=0.5)
    ds = DeviceTrainDataset(images, labels, hyp, img_size=s, batch_size=4, stride=16, device=dev, segments=segments, copy_paste=True)
    _seed(s)
    items = ds.draw_batch(0)
    st = cpc.batch_statement(items, images, labels, segments, hw, s)
    assert max(len(a) for a in st["accepted"]) > 4
    polys = [p for it in items for mo in it.mosaics for p in cpc.mosaic_rows(mo, labels, segments, hw)[1]]
    assert any((p == 0).any() and (p == 2 * s).any() for p in polys) and {1024, 1025, 1203} <= {len(p) for p in polys}
    im, targets, _, _ = ds.get_batch(0, items=items)
    _assert_pastes(ds, items, st, f"canvas {2 * s}")
    assert torch.equal(_bits(targets.cpu()), _bits(torch.from_numpy(st["targets"]))) and torch.equal(ds.polygons[2].cpu(), torch.from_numpy(st["words"]))
    assert torch.equal(im.cpu(), torch.from_numpy(st["im"]))


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float32])
def test_a_pasting_batch_in_the_floating_dtypes(data, dtype, dev):
    """the three other instantiations of the copy-paste sampler: the uint8 batch of the same items, x / 255 rounded once (what `im.to(dtype) / 255` gives, formed on the host: an IEEE division)"""
    c = CASES["wild_0.5"]
    u8, fl = _build(data, c["hyp"], dev, c["indices"], copy_paste=True), _build(data, c["hyp"], dev, c["indices"], copy_paste=True, dtype=dtype)
    _seed(c["seed"])
    items = u8.draw_batch(0)
    assert sum(len(mo.paste) for it in items for mo in it.mosaics) > 0
    want, got = u8.get_batch(0, items=items), fl.get_batch(0, items=items)
    assert fl.pastes is not None and got[0].dtype == dtype and torch.equal(got[0].cpu(), want[0].cpu().to(dtype) / 255) and torch.equal(_bits(got[1]), _bits(want[1]))
    assert not torch.equal(want[0], _build(data, dict(c["hyp"], copy_paste=0.0), dev, c["indices"]).get_batch(0, items=items)[0])   # and the pastes do change pixels


def test_the_keyword_with_p_zero_is_todays_batch(data, dev):
    c = apc.CASES["wild"]
    keyed, plain = _build(data, c["hyp"], dev, c["indices"], copy_paste=True), _build(data, c["hyp"], dev, c["indices"])
    assert keyed._poly_counts is None and keyed._stage.numel() == plain._stage.numel()   # no draw, the same staging buffer
    for k in range(len(plain)):
        _seed(c["seed"] + k)
        a = keyed.get_batch(k)
        after = random.random(), float(np.random.random())
        _seed(c["seed"] + k)
        b = plain.get_batch(k)
        assert (random.random(), float(np.random.random())) == after and keyed.pastes is None
        assert torch.equal(a[0], b[0]) and torch.equal(_bits(a[1]), _bits(b[1])) and a[2:] == b[2:]
        assert all(torch.equal(x, y) for x, y in zip(keyed.polygons, plain.polygons))


def test_a_box_only_set_and_a_letterbox_set_never_paste(data, dev):
    c = apc.CASES["wild"]
    hyp = dict(c["hyp"], copy_paste=0.5)
    for kw, base in ((dict(segments=None), dict(segments=None)), (dict(mosaic=False), dict(mosaic=False))):   # no polygons: no n; mosaic=False: load_mosaic never runs
        keyed, plain = _build(data, hyp, dev, copy_paste=True, **kw), _build(data, c["hyp"], dev, **base)
        _seed(9)
        a = keyed.get_batch(1)
        after = random.random(), float(np.random.random())
        _seed(9)
        b = plain.get_batch(1)
        assert (random.random(), float(np.random.random())) == after and keyed.pastes is None
        assert torch.equal(a[0], b[0]) and torch.equal(_bits(a[1]), _bits(b[1]))


def test_a_rect_batch_with_the_keyword_is_the_one_without(dev):
    from yolov3_amd import DeviceRectTrainDataset

    hyp = arc.CASES["rect_low"]["hyp"]
    args = dict(img_size=arc.IMG_SIZE, batch_size=arc.BATCH, stride=arc.STRIDE, shapes0=ac.hw0(), paths=ac.paths(), device=dev)
    keyed = DeviceRectTrainDataset(ac.make_images(), ac.make_labels(), dict(hyp, copy_paste=0.5), copy_paste=True, segments=apc.make_polygons()[1], **args)
    plain = DeviceRectTrainDataset(ac.make_images(), ac.make_labels(), hyp, **args)
    for k in range(len(plain)):
        _seed(k)
        a = keyed.get_batch(k)
        after = random.random(), float(np.random.random())
        _seed(k)
        b = plain.get_batch(k)
        assert (random.random(), float(np.random.random())) == after
        assert torch.equal(a[0], b[0]) and torch.equal(_bits(a[1]), _bits(b[1])) and a[2:] == b[2:]


def test_from_dataset_with_the_keyword_yields_a_pasted_batch(data, dev):
    from yolov3_amd import DeviceTrainDataset

    c = CASES["low_0.5"]
    ref = SimpleNamespace(ims=data.images, im_hw0=ac.hw0(), im_hw=ac.hw(), labels=data.labels, segments=data.segments, im_files=ac.paths(), rect=False, img_size=ac.IMG_SIZE,
                          stride=ac.STRIDE, augment=True, mosaic=True, hyp=dict(c["hyp"]), n=12, indices=range(12))
    ds = DeviceTrainDataset.from_dataset(ref, batch_size=ac.BATCH, device=dev, dtype=torch.float32, copy_paste=True)
    _seed(c["seed"])
    im, targets, paths, shapes = next(iter(ds))
    items_targets = torch.load(ROOT / "tests" / "golden" / "augment_copy_paste.pt", weights_only=True)["cases"]["low_0.5"]["batches"][0]["targets"]
    assert im.shape == (4, 3, 64, 64) and im.dtype == torch.float32 and ds.pastes is not None and torch.equal(_bits(targets.cpu()), _bits(items_targets))
