"""CPU tests of polygon labels in the train-mode dataset (yolov3_amd/augment.py, csrc/augment.hip): the NumPy statement of the polygon label path
(tests/augment_polygon_cases.py) against the fixture of the unmodified reference (tests/golden/make_augment_polygons_golden.py) and, where the reference tree is
present, against the live reference; the packed vertex table; the header; the refusals, all raised before anything is uploaded."""
import random
import re
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

NEW_SYMBOLS = ["y3_augment_polygons", "y3_augment_targets_polygons"]


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


def test_the_cases_are_what_the_issue_lists(data):
    counts = [len(sg) for sg in data.segments]
    assert [len(lb) for lb in data.labels] == ac.LABEL_COUNTS and all(c in (0, n) for c, n in zip(counts, ac.LABEL_COUNTS))
    assert [i for i, (c, n) in enumerate(zip(counts, ac.LABEL_COUNTS)) if n and not c] == list(apc.BOX_ONLY) and ac.LABEL_COUNTS[6] == 0
    sizes = [len(p) for sg in data.segments for p in sg]
    assert max(sizes) == 1203 > apc.SAMPLES and sorted(set(sizes))[:3] == [1, 2, 3] and all(k <= 40 for k in sizes if k != 1203)
    assert not data.segments[apc.ZEROS[0]][apc.ZEROS[1]].any() and len(data.segments[apc.MIXED_ROW[0]][apc.MIXED_ROW[1]]) == 2
    assert len(apc.label_lines(apc.MIXED_ROW[0], data.labels, data.segments)[apc.MIXED_ROW[1]].split()) == 5   # written as a plain box row
    for lb, sg in zip(data.labels, data.segments):   # the labels of a polygon image are segments2boxes of its polygons, valid for the reference's parser
        assert lb.dtype == np.float32 and (lb >= 0).all() and (lb[:, 1:] <= 1).all() and len(np.unique(lb, axis=0)) == len(lb)
        assert not len(sg) or np.array_equal(lb[:, 1:], apc.segments2boxes(sg))


def test_resample_is_linspace_and_interp():
    """the two restated formulas against NumPy's own functions, bit for bit (what the device restates rests on this)"""
    rs = np.random.RandomState(5)
    for k in (1, 2, 3, 7, 40, 999, 1000, 1001, 1203):
        p = (rs.uniform(0, 128, (k, 2))).astype(np.float32)
        closed = np.concatenate([p, p[:1]], 0)
        t = np.linspace(0, len(closed) - 1, apc.SAMPLES)
        want = np.concatenate([np.interp(t, np.arange(len(closed)), closed[:, i]) for i in range(2)]).reshape(2, -1).T
        assert np.array_equal(apc.resample(p), want)


@pytest.mark.parametrize("case", list(apc.CASES))
def test_the_statement_reproduces_the_fixture(gold, data, case):
    from yolov3_amd import draw_item

    c, g = apc.CASES[case], gold["cases"][case]
    epoch = c["indices"] if c["indices"] is not None else list(range(len(ac.IMAGES)))
    assert g["indices"] == epoch
    random.seed(c["seed"])
    np.random.seed(c["seed"])
    for k, want in enumerate(g["batches"]):
        items = [draw_item(i, ac.hw(), c["hyp"], ac.IMG_SIZE, epoch, len(ac.IMAGES), True) for i in epoch[k * ac.BATCH : (k + 1) * ac.BATCH]]
        st = apc.batch_statement(items, data.labels, data.segments, ac.hw(), ac.IMG_SIZE)
        assert np.array_equal(st["targets"].view(np.int32), want["targets"].numpy().view(np.int32)), f"{case}: targets of batch {k}"
        assert np.array_equal(st["boxes"].view(np.int64), want["boxes"].numpy().view(np.int64)) and np.array_equal(st["inside"], want["inside"].numpy())
        assert np.array_equal(st["words"], want["words"].numpy()) and np.array_equal(st["written"], want["written"].numpy())
        assert np.array_equal(st["words"] == apc.PATH_NONZERO, want["reference_resampled"].numpy())   # the path the reference took
    state = random.getstate(), np.random.get_state()
    assert random.random() == g["batches"][-1]["next_random"] and float(np.random.random()) == g["batches"][-1]["next_np_random"]
    random.setstate(state[0])
    np.random.set_state(state[1])
    if case == "single":   # the letterbox branch hands no segments on: the box path on polygon data
        assert not any(b["words"].any() or b["written"].any() for b in g["batches"])
    else:
        words = torch.cat([b["words"].reshape(-1) for b in g["batches"]]).tolist()
        assert apc.PATH_NONZERO in words and (apc.PATH_NONZERO | apc.PATH_LACKS) in words


def test_the_statement_reproduces_the_live_reference(gold):
    from oracle import ref_shim

    if not ref_shim.available():
        pytest.skip("the reference tree is not readable here")
    sys.path.insert(0, str(ROOT / "tests" / "golden"))
    import tempfile

    import make_augment_golden as base
    import make_augment_polygons_golden as gen

    with tempfile.TemporaryDirectory() as tmp:   # run_case asserts, per item, statement == reference (targets, paths, fp32 boxes) and the images of the box-only run
        gen.write_tree(Path(tmp))
        live = gen.run_case(base.reference(), Path(tmp), "exact", gen.new_stats())
    g = gold["cases"]["exact"]
    assert live["indices"] == g["indices"] and len(live["batches"]) == len(g["batches"])
    for a, b in zip(live["batches"], g["batches"]):
        assert torch.equal(a["targets"], b["targets"]) and torch.equal(a["boxes"], b["boxes"]) and torch.equal(a["words"], b["words"]) and a["paths"] == b["paths"]
        assert torch.equal(a["reference_resampled"], b["reference_resampled"]) and a["next_random"] == b["next_random"]


def test_the_vertex_table_and_offsets(data):
    from yolov3_amd import augment

    vertices, offsets = augment.pack_polygons(data.labels, data.segments, ac.paths())
    rows = sum(ac.LABEL_COUNTS)
    assert vertices.dtype == np.float32 and vertices.flags["C_CONTIGUOUS"] and vertices.shape == (sum(len(p) for sg in data.segments for p in sg), 2)
    assert offsets.dtype == np.int64 and offsets.shape == (rows + 1,) and offsets[0] == 0 and offsets[-1] == len(vertices) and (np.diff(offsets) >= 0).all()
    r = 0
    for lb, sg in zip(data.labels, data.segments):
        for j in range(len(lb)):
            got = vertices[offsets[r] : offsets[r + 1]]
            assert np.array_equal(got, sg[j]) if len(sg) else len(got) == 0   # a row of a box-only image owns nothing
            r += 1
    assert r == rows
    v, o = augment.pack_polygons(data.labels, [[] for _ in data.labels])
    assert v.shape == (0, 2) and o.tolist() == [0] * (rows + 1)


def test_the_header_declares_the_new_exports_at_abi_6():
    from yolov3_amd import _lib, augment, ops

    header = (ROOT / "include" / "yolov3_hip.h").read_text()
    declared = set(re.findall(r"\b(y3_[a-z0-9_]+)\s*\(", header))
    assert set(NEW_SYMBOLS) <= declared and declared == set(_lib.exported_symbols())
    assert "#define Y3_ABI_VERSION 6" in re.sub(r"[ \t]+", " ", header) and _lib.ABI_VERSION == 6
    assert len(_lib._SIGNATURES["y3_augment_polygons"][1]) == 15 and len(_lib._SIGNATURES["y3_augment_targets_polygons"][1]) == 14
    assert len(_lib._SIGNATURES["y3_augment_targets"][1]) == 11   # the box form keeps its signature
    assert not ({"y3_augment_polygons", "y3_augment_targets_polygons"} & set(_lib._QUERIES))   # both launch: both end in `void* stream`
    assert (augment.TILE.itemsize, augment.MOSAIC.itemsize, augment.ITEM.itemsize) == (40, 280, 1360)   # the mosaic's decision lives in the workspace, not the record
    assert callable(ops.augment_polygons) and callable(ops.augment_targets_polygons)
    assert all(s in (ROOT / "INTEGRATION.md").read_text() for s in NEW_SYMBOLS)
    source = (ROOT / "yolov3_amd" / "csrc" / "augment.hip").read_text()
    assert all(f'extern "C" int {s}(' in source for s in NEW_SYMBOLS)


def test_the_new_exports_reject_bad_arguments_without_a_gpu():
    from yolov3_amd import _lib, build

    build.build(verbose=False)
    lib = _lib.lib()
    P = 1 << 20   # a fake, aligned device address: validation never dereferences it

    def fails(status, *needles):
        msg = lib.y3_last_error()
        assert status != 0 and all(n in msg for n in needles), (status, msg)

    def polygons(verts=P, nv=100, voff=P, rows=26, loff=P, images=P, n=12, items=P, count=4, S=64, boxes=P, inside=P, paths=P, n_rows=30):
        return lib.y3_augment_polygons(verts, nv, voff, rows, loff, images, n, items, count, S, boxes, inside, paths, n_rows, None)

    for null in ("verts", "voff", "loff", "images", "items", "boxes", "inside", "paths"):
        fails(polygons(**{null: None}), b"y3_augment_polygons", b"null")
    fails(polygons(nv=-1), b"y3_augment_polygons", b"geometry")
    fails(polygons(nv=1 << 31), b"y3_augment_polygons", b"geometry")
    fails(polygons(rows=-1), b"y3_augment_polygons", b"geometry")
    fails(polygons(n_rows=-1), b"y3_augment_polygons", b"geometry")
    fails(polygons(count=1025), b"y3_augment_polygons", b"geometry")
    fails(polygons(S=72), b"y3_augment_polygons", b"72 is not a multiple of 16")
    fails(polygons(voff=P + 4), b"y3_augment_polygons", b"aligned")
    fails(polygons(boxes=P + 4), b"y3_augment_polygons", b"aligned")
    fails(polygons(inside=P + 2), b"y3_augment_polygons", b"aligned")
    assert polygons(count=0, paths=None) == 0   # an empty batch launches nothing

    def targets(labels=P, loff=P, images=P, n=12, items=P, count=4, S=64, boxes=P, inside=P, paths=P, out=P, rows=5, out_offsets=P):
        return lib.y3_augment_targets_polygons(labels, loff, images, n, items, count, S, boxes, inside, paths, out, rows, out_offsets, None)

    for null in ("labels", "loff", "images", "items", "boxes", "inside", "paths", "out", "out_offsets"):
        fails(targets(**{null: None}), b"y3_augment_targets_polygons", b"null")
    fails(targets(rows=-1), b"y3_augment_targets_polygons", b"geometry")
    fails(targets(S=100), b"y3_augment_targets_polygons", b"100 is not a multiple of 16")
    fails(targets(boxes=P + 4), b"y3_augment_targets_polygons", b"aligned")
    fails(targets(paths=P + 2), b"y3_augment_targets_polygons", b"aligned")


def _ds(data, hyp=None, **kw):
    from yolov3_amd import DeviceTrainDataset

    args = dict(img_size=ac.IMG_SIZE, batch_size=ac.BATCH, stride=ac.STRIDE, shapes0=ac.hw0(), paths=ac.paths(), device="cpu", segments=data.segments)
    args.update(kw)
    return DeviceTrainDataset(data.images, args.pop("labels", data.labels), dict(ac.CASES["low"]["hyp"]) if hyp is None else hyp, **args)


def test_polygons_are_accepted_and_the_refusals_come_before_any_upload(data, monkeypatch):
    from yolov3_amd import dataset

    def no_upload(*a, **k):
        raise AssertionError("an upload was attempted")

    monkeypatch.setattr(dataset, "_upload", no_upload)
    monkeypatch.setattr(dataset, "_upload_arena", no_upload)
    with pytest.raises(RuntimeError, match="no CPU / PyTorch fallback"):   # a valid polygon set: the device is what is missing
        _ds(data)
    short = [list(sg) for sg in data.segments]
    short[1] = short[1][:3]   # image 000002: five label rows, three polygons
    with pytest.raises(ValueError, match=r"images/000002\.png holds 3 polygon labels for 5 label rows"):
        _ds(data, segments=short)
    extra = [list(sg) for sg in data.segments]
    extra[6] = [np.zeros((4, 2), dtype=np.float32)]   # the label-less image with a polygon
    with pytest.raises(ValueError, match=r"images/000007\.png holds 1 polygon labels for 0 label rows"):
        _ds(data, segments=extra)
    empty = [list(sg) for sg in data.segments]
    empty[0][1] = np.zeros((0, 2), dtype=np.float32)
    with pytest.raises(ValueError, match=r"images/000001\.png.*polygon labels has shape \(0, 2\)"):
        _ds(data, segments=empty)
    with pytest.raises(ValueError, match="polygon labels for 11 images"):
        _ds(data, segments=data.segments[:11])
    low = ac.CASES["low"]["hyp"]
    with pytest.raises(ValueError, match="copy_paste"):
        _ds(data, dict(low, copy_paste=0.1))
    with pytest.raises(ValueError, match="perspective"):
        _ds(data, dict(low, perspective=0.001))
    with pytest.raises(ValueError, match="rect=True"):
        _ds(data, rect=True)


def test_from_dataset_passes_polygons_through(data):
    from yolov3_amd import DeviceTrainDataset

    ref = SimpleNamespace(ims=data.images, im_hw0=ac.hw0(), im_hw=ac.hw(), labels=data.labels, segments=data.segments, im_files=ac.paths(), rect=False, img_size=64, stride=32,
                          augment=True, mosaic=True, hyp=dict(ac.CASES["low"]["hyp"]), indices=range(12))
    with pytest.raises(RuntimeError, match="no CPU"):   # read and accepted
        DeviceTrainDataset.from_dataset(ref, batch_size=4, device="cpu")
    ref.segments = [list(sg) for sg in data.segments]
    ref.segments[2] = ref.segments[2][:1]
    with pytest.raises(ValueError, match=r"images/000003\.png holds 1 polygon labels for 6 label rows"):   # the polygons did reach the constructor
        DeviceTrainDataset.from_dataset(ref, batch_size=4, device="cpu")


def test_cpu_tensors_are_refused():
    from yolov3_amd import ops

    z, items = torch.zeros(32 * 12, dtype=torch.uint8), torch.zeros(4 * 1360, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="no CPU"):
        ops.augment_polygons(torch.zeros(8, 2), torch.zeros(5, dtype=torch.int64), torch.zeros(13, dtype=torch.int64), z, 12, items, 4, 64, 4)
    with pytest.raises(RuntimeError, match="no CPU"):
        ops.augment_targets_polygons(torch.zeros(4, 5), torch.zeros(13, dtype=torch.int64), z, 12, items, 4, 64, 4, torch.zeros(4, 4, dtype=torch.float64),
                                     torch.zeros(4, dtype=torch.int32), torch.zeros(4, 2, dtype=torch.int32))
