"""CPU tests of the rect train-mode dataset (DeviceRectTrainDataset of yolov3_amd/augment.py, the _hw exports of csrc/augment.hip): the host side -- draw_item's random
stream, matrices, letterbox geometry, tables and flags for (H, W) items against the fixture of the unmodified reference (tests/golden/make_augment_rect_golden.py), the
packed record -- the NumPy statement of one rect item against the fixture's images and targets, the public surface, the C ABI's argument validation without a GPU,
and every refusal of the constructor (all raised before anything is uploaded, so none needs a device)."""
import random
import re
import struct
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

NEW_SYMBOLS = ["y3_augment_batch_hw", "y3_augment_targets_hw"]


@pytest.fixture(scope="module")
def lib():
    from yolov3_amd import _lib, build

    build.build(verbose=False)
    return _lib.lib()


@pytest.fixture(scope="module")
def gold(golden_dir):
    return torch.load(golden_dir / "augment_rect.pt", weights_only=True)   # data only


@pytest.fixture(scope="module")
def data():
    images, labels, hw, hw0, paths = arc.sorted_set()
    return SimpleNamespace(images=images, labels=labels, hw=hw, hw0=hw0, paths=paths, file_images=ac.make_images(), file_labels=ac.make_labels())


@pytest.fixture(autouse=True)
def _generators_left_alone():
    state = random.getstate(), np.random.get_state()
    yield
    random.setstate(state[0])
    np.random.set_state(state[1])


def _items(case, gold, check=None):
    """every batch of `case` drawn by draw_item from the case's seeds -> [(H, W, [Item])]; check(k, slot, item, want) sees every item as it is drawn"""
    from yolov3_amd import draw_item

    c, g = arc.CASES[case], gold["cases"][case]
    hw = [ac.hw()[i] for i in arc.file_index()]
    random.seed(c["seed"])
    np.random.seed(c["seed"])
    out = []
    for k, b in enumerate(g["batches"]):
        H, W = g["batch_shapes"][k]
        items = []
        for slot, want in enumerate(b["items"]):
            items.append(draw_item(k * arc.BATCH + slot, hw, c["hyp"], (H, W), None, len(ac.IMAGES), False))
            if check is not None:
                check(k, slot, items[-1], want)
        state = random.getstate(), np.random.get_state()
        assert random.random() == b["next_random"] and float(np.random.random()) == b["next_np_random"], f"{case}: batch {k} leaves the generators elsewhere"
        random.setstate(state[0])
        np.random.set_state(state[1])
        out.append((H, W, items))
    return out


def test_public_names_import():
    import yolov3_amd
    from yolov3_amd import DeviceDataset, DeviceRectTrainDataset, DeviceTrainDataset, augment, ops

    assert augment.DeviceRectTrainDataset is DeviceRectTrainDataset and issubclass(DeviceRectTrainDataset, DeviceDataset) and not issubclass(DeviceRectTrainDataset, DeviceTrainDataset)
    assert callable(DeviceRectTrainDataset.from_dataset) and callable(ops.augment_batch_hw) and callable(ops.augment_targets_hw)
    assert "DeviceRectTrainDataset" in yolov3_amd.__doc__ and "DeviceRectTrainDataset" in augment.__doc__
    assert all("DeviceRectTrainDataset" in (ROOT / f).read_text() for f in ("README.md", "DESIGN.md", "INTEGRATION.md"))
    assert "augment_rect_ab.py" in (ROOT / "tools" / "README.md").read_text()


def test_the_two_exports_are_declared_bound_and_exported_at_abi_6(lib):
    from yolov3_amd import _lib, augment, ops

    header = (ROOT / "include" / "yolov3_hip.h").read_text()
    declared = set(re.findall(r"\b(y3_[a-z0-9_]+)\s*\(", header))
    assert set(NEW_SYMBOLS) <= declared and set(NEW_SYMBOLS) <= set(_lib.exported_symbols()) and declared == set(_lib.exported_symbols())
    assert {"y3_augment_batch", "y3_augment_targets", "y3_augment_polygons", "y3_augment_targets_polygons"} <= declared   # the four square exports stay
    assert "#define Y3_ABI_VERSION 6" in re.sub(r"[ \t]+", " ", header) and lib.y3_abi_version() == 6 == _lib.ABI_VERSION
    assert ("augment.hip", ["-ffp-contract=off"]) in __import__("yolov3_amd.build", fromlist=["SOURCES"]).SOURCES
    assert all(hasattr(lib, s) and s in _lib._SIGNATURES for s in NEW_SYMBOLS)   # bound from the header, no table of its own
    assert (augment.TILE.itemsize, augment.MOSAIC.itemsize, augment.ITEM.itemsize) == (40, 280, 1360) == (40, 280, ops.AUGMENT_ITEM_BYTES)
    # the offsets of every field the records had, and the two words that were spare
    assert [augment.MOSAIC.fields[n][1] for n in ("inv", "m", "scale", "ntiles", "canvas", "clip", "canvas_h", "tiles")] == [0, 48, 96, 104, 108, 112, 116, 120]
    assert [augment.TILE.fields[n][1] for n in ("img", "x1", "y1", "x2", "y2", "padw", "padh", "lpadw", "lpadh", "wide")] == [0, 4, 8, 12, 16, 20, 24, 28, 32, 36]
    assert [augment.ITEM.fields[n][1] for n in ("mosaics", "ratio", "ratio1", "nmos", "flipud", "fliplr", "hsv", "lut")] == [0, 560, 568, 576, 580, 584, 588, 592]


def test_the_hw_exports_reject_bad_arguments_without_a_gpu(lib):
    P = 1 << 20   # a fake, aligned device address: validation never dereferences it
    U8, F16 = 3, 0

    def fails(status, *needles):
        msg = lib.y3_last_error()
        assert status != 0 and all(n in msg for n in needles), (status, msg)

    def batch(arena=P, arena_bytes=4096, images=P, n=12, items=P, count=4, dst=P, dtype=U8, H=48, W=64):
        return lib.y3_augment_batch_hw(arena, arena_bytes, images, n, items, count, dst, dtype, H, W, None)

    name = b"y3_augment_batch_hw"
    for kw in (dict(arena=None), dict(images=None), dict(items=None), dict(dst=None)):
        fails(batch(**kw), name, b"null")
    for kw in (dict(n=0), dict(count=-1), dict(count=1025), dict(H=0), dict(W=0), dict(H=4112), dict(W=4112), dict(H=-16)):
        fails(batch(**kw), name, b"geometry")
    fails(batch(H=72), name, b"72 is not a multiple of 16")
    fails(batch(W=40), name, b"40 is not a multiple of 16")
    fails(batch(items=P + 4), name, b"8-byte aligned")
    fails(batch(arena_bytes=4098), name, b"multiple of 4")
    fails(batch(arena=P + 8), name, b"16-byte aligned")
    fails(batch(dst=P + 8, dtype=F16), name, b"16-byte aligned")
    fails(batch(dtype=7), name, b"unsupported output dtype 7")
    assert batch(count=0) == 0 and batch(count=0, H=4096, W=16) == 0   # an empty batch launches nothing

    def targets(labels=P, offsets=P, images=P, n=12, items=P, count=4, H=64, W=48, out=P, rows=5, out_offsets=P):
        return lib.y3_augment_targets_hw(labels, offsets, images, n, items, count, H, W, out, rows, out_offsets, None)

    name = b"y3_augment_targets_hw"
    for kw in (dict(offsets=None), dict(out_offsets=None), dict(labels=None), dict(out=None), dict(images=None), dict(items=None)):
        fails(targets(**kw), name, b"null")
    for kw in (dict(n=-2), dict(count=1025), dict(rows=-1), dict(rows=1 << 31), dict(H=8), dict(W=8192)):
        fails(targets(**kw), name, b"geometry")
    fails(targets(H=100), name, b"100 is not a multiple of 16")
    fails(targets(W=24), name, b"24 is not a multiple of 16")
    for kw in (dict(offsets=P + 4), dict(out_offsets=P + 4), dict(labels=P + 2), dict(items=P + 4)):
        fails(targets(**kw), name, b"aligned")
    # the square exports still name themselves
    fails(lib.y3_augment_batch(P, 4096, P, 12, P, 4, P, U8, 72, None), b"y3_augment_batch:", b"72 is not a multiple of 16")
    fails(lib.y3_augment_targets(P, P, P, 12, P, 4, 100, P, 5, P, None), b"y3_augment_targets:", b"100 is not a multiple of 16")


def test_the_fixture_holds_the_layout_and_the_situations(gold, data):
    from yolov3_amd.dataset import layout, rect_batch_shapes

    assert list(gold["cases"]) == list(arc.CASES) and abs(ac.checksum(data.file_images, data.file_labels) - gold["checksum"]) < 1e-6
    order, batch, shapes = rect_batch_shapes([(w0, h0) for h0, w0 in ac.hw0()], arc.IMG_SIZE, arc.BATCH, arc.STRIDE, 0.0)
    for g in gold["cases"].values():
        assert g["order"] == [int(i) for i in order] == arc.file_index() and g["batch"] == [int(b) for b in batch]
        assert g["batch_shapes"] == [tuple(int(v) for v in s) for s in shapes] == arc.BATCH_SHAPES == [(48, 64), (64, 64), (64, 48)]
    assert [Path(p).stem for p in data.paths] == arc.ORDER
    lay = layout(ac.hw(), ac.hw0(), arc.IMG_SIZE, arc.BATCH, arc.STRIDE, 0.0, True, ac.paths())
    halves = [s[1][1] for s in lay.shapes]
    assert {5.5, 1.5} <= {dh for _, dh in halves} and {3.5, 7.5, 12.5} <= {dw for dw, _ in halves}   # letterbox halves ending in .5 on both axes
    assert all(min(H / h, W / w) == 1.0 for (h, w), (H, W) in zip(data.hw, (arc.BATCH_SHAPES[b] for b in batch)))   # r = 1: no resize
    assert [len(lb) for lb in data.labels[:4]].count(0) == 1   # the label-less image, in the wide batch
    assert len({tuple(s) for s in rect_batch_shapes([(w0, h0) for h0, w0 in ac.hw0()], arc.IMG_SIZE, arc.BATCH, 32, 0.0)[2].tolist()}) == 1   # stride 32 pins nothing
    items = {c: [(k, it) for k, b in enumerate(g["batches"]) for it in b["items"]] for c, g in gold["cases"].items()}
    flips = {(k != 1, it["flipud"], it["fliplr"]) for v in items.values() for k, it in v}
    assert all(any(f[0] and f[axis] == on for f in flips) for axis in (1, 2) for on in (True, False))   # each flip on and off in a batch that is not square
    eye = torch.eye(3, dtype=torch.float64)
    assert all(torch.equal(it["M"], eye) and it["luts"] is None for _, it in items["rect_exact"]) and not any(torch.equal(it["M"], eye) for _, it in items["rect_low"])
    assert all("im" not in b for b in gold["cases"]["rect_low_f16"]["batches"]) and all(tuple(b["im"].shape) == (4, 3, *arc.BATCH_SHAPES[k]) for k, b in
                                                                                        enumerate(gold["cases"]["rect_low"]["batches"]))


@pytest.mark.parametrize("case", list(arc.CASES))
def test_draw_item_is_the_reference_stream_for_rect_items(gold, data, case):
    def check(k, slot, it, want):
        H, W = arc.BATCH_SHAPES[k]
        mo = it.mosaics[0]
        (h, w), where = data.hw[it.index], f"{case} batch {k} item {slot}"
        assert (it.index, it.mosaic, it.flipud, it.fliplr, it.ratio, len(it.mosaics)) == (want["index"], False, want["flipud"], want["fliplr"], None, 1), where
        assert (it.luts is None) == (want["luts"] is None) and (it.luts is None or np.array_equal(it.luts, want["luts"].numpy())), where
        assert mo.M.dtype == np.float64 and mo.M.tobytes() == want["M"].numpy().tobytes(), f"{where}: M\n{mo.M}\n{want['M']}"
        assert mo.scale == want["scale"] and tuple(mo.rects[0]) == want["rect"] and tuple(mo.pad[0]) == want["pad"] == ((W - w) / 2, (H - h) / 2), where
        assert (mo.canvas, mo.canvas_h, mo.indices) == (W, H, [it.index]) and mo.rects[0][:4] == (round((W - w) / 2 - 0.1), round((H - h) / 2 - 0.1), round((W - w) / 2 - 0.1) + w,
                                                                                                 round((H - h) / 2 - 0.1) + h), where

    assert len(_items(case, gold, check)) == 3


def test_the_square_call_forms_draw_what_they_drew(data):
    """an int img_size is the square item of DeviceTrainDataset: the same draws, the same matrix, no canvas_h; a pair of equal sides is a rect item of a square batch"""
    from yolov3_amd import augment

    hyp = arc.CASES["rect_wild"]["hyp"]
    got = []
    for size in (64, (64, 64)):
        random.seed(3)
        np.random.seed(3)
        got.append(augment.draw_item(5, data.hw, hyp, size, None, 12, False))
    a, b = got
    assert a.mosaics[0].M.tobytes() == b.mosaics[0].M.tobytes() and a.mosaics[0].rects == b.mosaics[0].rects and (a.flipud, a.fliplr) == (b.flipud, b.fliplr)
    assert a.mosaics[0].canvas_h is None and b.mosaics[0].canvas_h == 64 and np.array_equal(a.luts, b.luts)
    random.seed(3)
    M, s = augment.draw_perspective(hyp, 64, 0)
    random.seed(3)
    M2, s2 = augment.draw_perspective(hyp, (48, 64), 0)
    assert s == s2 and np.array_equal(M[0, :2], M2[0, :2]) and M.tobytes() == a.mosaics[0].M.tobytes() and not np.array_equal(M[1], M2[1])
    with pytest.raises(ValueError, match="load_mosaic is square"):
        augment.draw_item(0, data.hw, hyp, (48, 64), None, 12, True)
    ra, rb = augment.pack_items([a]), augment.pack_items([b])
    assert struct.unpack_from("<d4i", ra.tobytes(), 96) == (a.mosaics[0].scale, 1, 64, 0, 0) and struct.unpack_from("<d4i", rb.tobytes(), 96) == (b.mosaics[0].scale, 1, 64, 0, 64)
    assert struct.unpack_from("<i", ra.tobytes(), 120 + 36) == (0,) and struct.unpack_from("<i", rb.tobytes(), 120 + 36) == (1,)


def test_the_packed_rect_record(data):
    from yolov3_amd import augment

    M = np.array([[1.25, -0.5, 3.0], [0.25, 0.75, -7.0], [0, 0, 1]], dtype=np.float64)
    mo = augment.Mosaic([2], [(0, 5, 64, 42, 0, 0, 64, 37)], M, 1.5, 64, [(0.0, 5.5)], None, 48)
    raw = augment.pack_items([augment.Item(2, [mo], None, None, True, True, False)]).tobytes()
    assert len(raw) == 1360 and struct.unpack_from("<6d", raw, 48) == (1.25, -0.5, 3.0, 0.25, 0.75, -7.0)
    assert struct.unpack_from("<d4i", raw, 96) == (1.5, 1, 64, 0, 48)   # ntiles, canvas (the width), clip, canvas_h
    assert struct.unpack_from("<7i2fi", raw, 120) == (2, 0, 5, 64, 42, 0, 5, 0.0, 5.5, 1)   # the tile: ..., lpadw, lpadh, wide
    assert struct.unpack_from("<2d4i", raw, 560) == (0.0, 0.0, 1, 1, 1, 0) and raw[280:560] == bytes(280)


@pytest.mark.parametrize("case", [c for c in arc.CASES if c not in arc.IMAGES_OF])
def test_the_numpy_statement_of_a_rect_item_is_the_fixture(gold, data, case):
    for k, (H, W, items) in enumerate(_items(case, gold)):
        want = gold["cases"][case]["batches"][k]
        im = np.stack([arc.item_image(it, data.images, H, W) for it in items])
        assert np.array_equal(im, want["im"].numpy()), f"{case}: images of batch {k}"
        assert np.array_equal(arc.batch_targets(items, data.labels, data.hw, H, W).view(np.int32), want["targets"].numpy().view(np.int32)), f"{case}: targets of batch {k}"
        assert want["paths"] == [data.paths[it.index] for it in items]
        assert want["shapes"] == tuple((data.hw0[it.index], ((data.hw[it.index][0] / data.hw0[it.index][0], data.hw[it.index][1] / data.hw0[it.index][1]), it.mosaics[0].pad[0]))
                                       for it in items)


def _ds(data, hyp=None, **kw):
    from yolov3_amd import DeviceRectTrainDataset

    args = dict(img_size=arc.IMG_SIZE, batch_size=arc.BATCH, stride=arc.STRIDE, shapes0=ac.hw0(), paths=ac.paths(), device="cpu")
    args.update(kw)
    return DeviceRectTrainDataset(args.pop("images", data.file_images), args.pop("labels", data.file_labels), dict(arc.CASES["rect_low"]["hyp"]) if hyp is None else hyp, **args)


def test_every_new_refusal_comes_before_any_upload(data, monkeypatch):
    from yolov3_amd import dataset

    def no_upload(*a, **k):
        raise AssertionError("an upload was attempted")

    monkeypatch.setattr(dataset, "_upload", no_upload)
    monkeypatch.setattr(dataset, "_upload_arena", no_upload)
    low = arc.CASES["rect_low"]["hyp"]
    with pytest.raises(RuntimeError, match="no CPU / PyTorch fallback"):   # valid inputs, a CPU device
        _ds(data)
    with pytest.raises(RuntimeError, match="no CPU"):   # segments are accepted and not used
        _ds(data, segments=[[np.zeros((5, 2), dtype=np.float32)] * len(lb) for lb in data.file_labels])
    with pytest.raises(ValueError, match="perspective.*warpPerspective is not built"):
        _ds(data, dict(low, perspective=0.001))
    with pytest.raises(ValueError, match="copy_paste.*copy-paste is not built"):
        _ds(data, dict(low, copy_paste=0.1))
    small = list(data.file_images)
    small[4] = np.zeros((40, 50, 3), dtype=np.uint8)   # letterbox(scaleup=True) would scale it up: r = 1.28
    with pytest.raises(ValueError, match=r"image images/000005.png is 40x50 and its batch shape 64x64.*r != 1.*cv2.resize"):
        _ds(data, images=small)
    large = list(data.file_images)
    large[6] = np.zeros((20, 80, 3), dtype=np.uint8)   # wider than its batch: r = 0.8
    with pytest.raises(ValueError, match=r"image images/000007.png is 20x80 and its batch shape 48x64.*cv2.resize"):
        _ds(data, images=large)
    for bad in (63, 72, 8):
        with pytest.raises(ValueError, match=f"img_size = {bad} must be a multiple of 16"):
            _ds(data, img_size=bad)
    for bad in (8, 24, 40):
        with pytest.raises(ValueError, match=f"stride = {bad} must be a multiple of 16"):
            _ds(data, stride=bad)
    for key in ("mosaic", "mixup", "degrees", "translate", "scale", "shear", "perspective", "hsv_h", "hsv_s", "hsv_v", "flipud", "fliplr", "copy_paste"):
        with pytest.raises(KeyError, match=key):
            _ds(data, {k: v for k, v in low.items() if k != key})
    with pytest.raises(TypeError, match="float64"):   # the shared constructor's refusals still apply
        _ds(data, dtype=torch.float64)
    with pytest.raises(ValueError, match="12 images, but 11 label arrays"):
        _ds(data, labels=data.file_labels[:11])


def test_from_dataset_reads_a_rect_reference_dataset(data, gold, monkeypatch):
    from yolov3_amd import DeviceDataset, DeviceRectTrainDataset, dataset

    monkeypatch.setattr(dataset, "_upload", lambda *a, **k: (_ for _ in ()).throw(AssertionError("an upload was attempted")))
    g = gold["cases"]["rect_low"]
    ref = SimpleNamespace(ims=data.images, im_hw0=data.hw0, im_hw=data.hw, labels=data.labels, segments=[[]] * 12, im_files=data.paths, rect=True, img_size=64, stride=16,
                          augment=True, mosaic=False, hyp=dict(arc.CASES["rect_low"]["hyp"]), indices=range(12), batch=np.array(g["batch"]), batch_shapes=np.array(g["batch_shapes"]))
    with pytest.raises(RuntimeError, match="no CPU"):   # everything read and accepted: the device is what is missing
        DeviceRectTrainDataset.from_dataset(ref, batch_size=4, device="cpu")
    with pytest.raises(ValueError, match="not built for 12 images in batches of 3"):   # the adopted batch index belongs to its batch size
        DeviceRectTrainDataset.from_dataset(ref, batch_size=3, device="cpu")
    ref.hyp["perspective"] = 0.5
    with pytest.raises(ValueError, match="perspective"):
        DeviceRectTrainDataset.from_dataset(ref, batch_size=4, device="cpu")
    ref.hyp["perspective"], ref.rect = 0.0, False
    with pytest.raises(ValueError, match="rect=False.*DeviceTrainDataset"):
        DeviceRectTrainDataset.from_dataset(ref, batch_size=4, device="cpu")
    ref.rect, ref.augment = True, False
    with pytest.raises(ValueError, match="does not augment"):
        DeviceRectTrainDataset.from_dataset(ref, batch_size=4, device="cpu")
    ref.augment, ref.ims = True, [None] * 12
    with pytest.raises(ValueError, match='cache="ram"'):
        DeviceRectTrainDataset.from_dataset(ref, batch_size=4, device="cpu")
    assert DeviceRectTrainDataset.set_indices is DeviceDataset.set_indices   # a rect set keeps its order: the shared refusal (raised on the device in the GPU tests)


def test_the_three_old_refusals_still_stand(data):
    from yolov3_amd import DeviceDataset, DeviceTrainDataset

    with pytest.raises(ValueError, match="rect=True.*mosaic = augment and not rect.*DeviceRectTrainDataset"):
        DeviceTrainDataset(data.file_images, data.file_labels, dict(ac.CASES["low"]["hyp"]), img_size=64, batch_size=4, shapes0=ac.hw0(), paths=ac.paths(), device="cpu", rect=True)
    ref = SimpleNamespace(ims=data.images, im_hw0=data.hw0, im_hw=data.hw, labels=data.labels, segments=[[]] * 12, im_files=data.paths, rect=True, img_size=64, stride=16,
                          augment=True, mosaic=False, hyp=dict(ac.CASES["low"]["hyp"]), indices=range(12))
    with pytest.raises(ValueError, match="rect=True"):
        DeviceTrainDataset.from_dataset(ref, batch_size=4, device="cpu")
    with pytest.raises(ValueError, match="augment"):
        DeviceDataset.from_dataset(ref, batch_size=4, device="cpu")


def test_cpu_tensors_are_refused():
    from yolov3_amd import ops

    z = torch.zeros(32 * 12, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="no CPU"):
        ops.augment_batch_hw(z, z, 12, torch.zeros(4 * 1360, dtype=torch.uint8), 4, 48, 64)
    with pytest.raises(RuntimeError, match="no CPU"):
        ops.augment_targets_hw(torch.zeros(4, 5), torch.zeros(13, dtype=torch.int64), z, 12, torch.zeros(4 * 1360, dtype=torch.uint8), 4, 48, 64, 4)


def test_golden_is_what_the_live_reference_computes(gold):
    from oracle import ref_shim

    if not ref_shim.available():
        pytest.skip("the reference tree is not readable here")
    sys.path.insert(0, str(ROOT / "tests" / "golden"))
    import tempfile

    import make_augment_golden as gen
    import make_augment_rect_golden as rect

    d = gen.reference()
    stats = rect.new_stats()
    for case in arc.CASES:
        with tempfile.TemporaryDirectory() as tmp:
            gen.write_tree(Path(tmp))
            live = rect.STORED[case] = rect.run_case(d, Path(tmp), case, stats)
        g = gold["cases"][case]
        assert (live["order"], live["batch"], live["batch_shapes"]) == (g["order"], g["batch"], g["batch_shapes"]) and len(live["batches"]) == len(g["batches"])
        for a, b in zip(live["batches"], g["batches"]):
            assert ("im" in a) == ("im" in b) and ("im" not in a or torch.equal(a["im"], b["im"])) and torch.equal(a["targets"], b["targets"])
            assert a["shapes"] == b["shapes"] and a["paths"] == b["paths"] and a["next_random"] == b["next_random"] and a["next_np_random"] == b["next_np_random"]
            assert all(torch.equal(x["M"], y["M"]) and x["rect"] == y["rect"] and x["pad"] == y["pad"] and (x["flipud"], x["fliplr"]) == (y["flipud"], y["fliplr"])
                       for x, y in zip(a["items"], b["items"]))
    rect.check_situations(stats)
