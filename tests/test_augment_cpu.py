"""CPU tests of the train-mode dataset (csrc/augment.hip, yolov3_amd/augment.py): the host side -- draw_item's random stream, matrices, rectangles, tables, flags and
ratios against the fixture of the unmodified reference (tests/golden/make_augment_golden.py), the packed record against a hand-decoded one -- the public surface, the
C ABI's argument validation without a GPU, and every refusal of the constructor (all raised before anything is uploaded, so none needs a device)."""
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

NEW_SYMBOLS = ["y3_augment_batch", "y3_augment_targets"]


@pytest.fixture(scope="module")
def lib():
    from yolov3_amd import _lib, build

    build.build(verbose=False)
    return _lib.lib()


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


def test_public_names_import():
    import yolov3_amd
    from yolov3_amd import DeviceDataset, DeviceTrainDataset, augment, draw_item, ops

    assert augment.DeviceTrainDataset is DeviceTrainDataset and issubclass(DeviceTrainDataset, DeviceDataset) and augment.draw_item is draw_item
    assert callable(DeviceTrainDataset.from_dataset) and callable(ops.augment_batch) and callable(ops.augment_targets)
    assert "DeviceTrainDataset" in yolov3_amd.__doc__ and "draw_item" in yolov3_amd.__doc__


def test_new_symbols_are_declared_bound_and_exported_at_abi_6(lib):
    from yolov3_amd import _lib, augment, ops

    header = (ROOT / "include" / "yolov3_hip.h").read_text()
    declared = set(re.findall(r"\b(y3_[a-z0-9_]+)\s*\(", header))
    assert set(NEW_SYMBOLS) <= declared and set(NEW_SYMBOLS) <= set(_lib.exported_symbols()) and declared == set(_lib.exported_symbols())
    assert "#define Y3_ABI_VERSION 6" in re.sub(r"[ \t]+", " ", header) and lib.y3_abi_version() == 6 == _lib.ABI_VERSION
    assert ("augment.hip", ["-ffp-contract=off"]) in __import__("yolov3_amd.build", fromlist=["SOURCES"]).SOURCES
    assert all(s in (ROOT / "INTEGRATION.md").read_text() for s in NEW_SYMBOLS + ["DeviceTrainDataset"])
    source = (ROOT / "yolov3_amd" / "augment.py").read_text()
    assert "_lib" not in source and "ctypes" not in source   # the module marshals no C call itself
    assert not re.search(r"\b(F\.pad|F\.grid_sample|torch\.(stack|cat|flip|clamp|where|nn))\b", source)   # no torch compute stands in for a kernel
    assert (augment.TILE.itemsize, augment.MOSAIC.itemsize, augment.ITEM.itemsize) == (40, 280, 1360) == (40, 280, ops.AUGMENT_ITEM_BYTES)
    assert all(f"}} {name};" in header for name in ("y3_augment_tile", "y3_augment_mosaic", "y3_augment_item"))


def test_new_exports_reject_bad_arguments_without_a_gpu(lib):
    P = 1 << 20   # a fake, aligned device address: validation never dereferences it
    U8, F16 = 3, 0

    def fails(status, *needles):
        msg = lib.y3_last_error()
        assert status != 0 and all(n in msg for n in needles), (status, msg)

    def batch(arena=P, arena_bytes=4096, images=P, n=12, items=P, count=4, dst=P, dtype=U8, S=64):
        return lib.y3_augment_batch(arena, arena_bytes, images, n, items, count, dst, dtype, S, None)

    fails(batch(arena=None), b"y3_augment_batch", b"null")
    fails(batch(images=None), b"y3_augment_batch", b"null")
    fails(batch(items=None), b"y3_augment_batch", b"null")
    fails(batch(dst=None), b"y3_augment_batch", b"null")
    fails(batch(n=0), b"y3_augment_batch", b"geometry")
    fails(batch(count=-1), b"y3_augment_batch", b"geometry")
    fails(batch(count=1025), b"y3_augment_batch", b"geometry")
    fails(batch(S=0), b"y3_augment_batch", b"geometry")
    fails(batch(S=4112), b"y3_augment_batch", b"geometry")
    fails(batch(S=72), b"y3_augment_batch", b"72 is not a multiple of 16")
    fails(batch(items=P + 4), b"y3_augment_batch", b"8-byte aligned")
    fails(batch(images=P + 4), b"y3_augment_batch", b"8-byte aligned")
    fails(batch(arena_bytes=4098), b"y3_augment_batch", b"multiple of 4")
    fails(batch(arena_bytes=0), b"y3_augment_batch", b"multiple of 4")
    fails(batch(arena=P + 8), b"y3_augment_batch", b"16-byte aligned")
    fails(batch(dst=P + 8, dtype=F16), b"y3_augment_batch", b"16-byte aligned")
    fails(batch(dtype=7), b"y3_augment_batch", b"unsupported output dtype 7")
    assert batch(count=0) == 0   # an empty batch launches nothing

    def targets(labels=P, offsets=P, images=P, n=12, items=P, count=4, S=64, out=P, rows=5, out_offsets=P):
        return lib.y3_augment_targets(labels, offsets, images, n, items, count, S, out, rows, out_offsets, None)

    fails(targets(offsets=None), b"y3_augment_targets", b"null")
    fails(targets(out_offsets=None), b"y3_augment_targets", b"null")
    fails(targets(labels=None), b"y3_augment_targets", b"null")
    fails(targets(out=None), b"y3_augment_targets", b"null")
    fails(targets(images=None), b"y3_augment_targets", b"null")
    fails(targets(items=None), b"y3_augment_targets", b"null")
    fails(targets(n=-2), b"y3_augment_targets", b"geometry")
    fails(targets(S=100), b"y3_augment_targets", b"100 is not a multiple of 16")
    fails(targets(count=1025), b"y3_augment_targets", b"geometry")
    fails(targets(rows=-1), b"y3_augment_targets", b"geometry")
    fails(targets(rows=1 << 31), b"y3_augment_targets", b"geometry")
    fails(targets(offsets=P + 4), b"y3_augment_targets", b"aligned")
    fails(targets(out_offsets=P + 4), b"y3_augment_targets", b"aligned")
    fails(targets(labels=P + 2), b"y3_augment_targets", b"aligned")
    fails(targets(items=P + 4), b"y3_augment_targets", b"aligned")


def test_case_builders_reproduce_the_golden(gold, data):
    assert list(gold["cases"]) == list(ac.CASES) and abs(ac.checksum(data.images, data.labels) - gold["checksum"]) < 1e-6
    assert [im.shape for im in data.images] == [(h, w, 3) for h, w in ac.hw()] and all(max(im.shape[:2]) == ac.IMG_SIZE and im.dtype == np.uint8 for im in data.images)
    assert [len(lb) for lb in data.labels] == ac.LABEL_COUNTS and 0 in ac.LABEL_COUNTS and max(ac.LABEL_COUNTS) == 6
    assert [len(c["batches"]) for c in gold["cases"].values()] == [3, 3, 4, 3, 3] and all(len(b["paths"]) == 4 for c in gold["cases"].values() for b in c["batches"])
    items = [it for c in gold["cases"].values() for b in c["batches"] for it in b["items"]]
    assert any(it["ratio"] is not None for it in items) and {(it["flipud"], it["fliplr"]) for it in items} == {(False, False), (True, False), (False, True), (True, True)}
    assert all(it["mosaic"] for it in gold["cases"]["wild"]["batches"][0]["items"]) and not any(it["mosaic"] for b in gold["cases"]["single"]["batches"] for it in b["items"])
    assert all(s is None for s in gold["cases"]["low"]["batches"][0]["shapes"]) and all(s is not None for s in gold["cases"]["single"]["batches"][0]["shapes"])
    for b in gold["cases"]["exact"]["batches"]:   # a translation by the whole number -s / 2 and nothing else
        for it in b["items"]:
            assert all(torch.equal(mo["M"], torch.tensor([[1.0, 0, -32], [0, 1, -32], [0, 0, 1]], dtype=torch.float64)) for mo in it["mosaics"]) and it["luts"] is None


def test_the_two_statements_on_values_worked_by_hand():
    # identity and whole-pixel translation: the plain copy / crop with a 114 border
    src = np.arange(5 * 7 * 3, dtype=np.uint8).reshape(5, 7, 3)
    assert np.array_equal(ac.warp_affine_u8(src, np.array([[1.0, 0, 0], [0, 1, 0]]), (7, 5)), src)
    out = ac.warp_affine_u8(src, np.array([[1.0, 0, 2], [0, 1, -1]]), (7, 5))
    assert np.array_equal(out[:4, 2:], src[1:, :5]) and (out[4] == 114).all() and (out[:, :2] == 114).all()
    # half a pixel to the right: fx = 16, the mean of two neighbours, + 512 >> 10 of weights 16 * 32
    g = np.array([[[10, 10, 10], [20, 20, 20], [41, 41, 41]]], dtype=np.uint8)
    assert ac.warp_affine_u8(g, np.array([[1.0, 0, 0.5], [0, 1, 0]]), (3, 1))[0, :, 0].tolist() == [(114 * 512 + 10 * 512 + 512) >> 10, 15, (20 * 512 + 41 * 512 + 512) >> 10]
    # pure colours and greys through both conversions
    px = np.array([[[255, 0, 0], [0, 255, 0], [0, 0, 255], [90, 90, 90], [0, 0, 0], [255, 255, 255]]], dtype=np.uint8)   # BGR: blue, green, red, grey, black, white
    assert ac.bgr2hsv_u8(px)[0].tolist() == [[120, 255, 255], [60, 255, 255], [0, 255, 255], [0, 0, 90], [0, 0, 0], [0, 0, 255]]
    assert np.array_equal(ac.hsv2bgr_u8(ac.bgr2hsv_u8(px)), px)


@pytest.mark.parametrize("case", list(ac.CASES))
def test_draw_item_is_the_reference_stream(gold, case):
    from yolov3_amd import draw_item

    c, g = ac.CASES[case], gold["cases"][case]
    epoch = c["indices"] if c["indices"] is not None else list(range(len(ac.IMAGES)))
    assert g["indices"] == epoch
    random.seed(c["seed"])
    np.random.seed(c["seed"])
    for k, b in enumerate(g["batches"]):   # (the generators are restored by the autouse fixture above)
        for slot, want in enumerate(b["items"]):
            it = draw_item(epoch[k * ac.BATCH + slot], ac.hw(), c["hyp"], ac.IMG_SIZE, epoch, len(ac.IMAGES), True)
            assert (it.index, it.mosaic, it.flipud, it.fliplr, it.ratio) == (want["index"], want["mosaic"], want["flipud"], want["fliplr"], want["ratio"])
            assert (it.luts is None) == (want["luts"] is None) and (it.luts is None or np.array_equal(it.luts, want["luts"].numpy()))
            assert len(it.mosaics) == len(want["mosaics"]) == 1 + (it.ratio is not None)
            for mo, w in zip(it.mosaics, want["mosaics"]):
                assert mo.M.dtype == np.float64 and mo.M.tobytes() == w["M"].numpy().tobytes(), f"{case} batch {k} item {slot}: M\n{mo.M}\n{w['M']}"
                assert mo.indices == w["indices"] and tuple(tuple(r) for r in mo.rects) == w["rects"] and mo.scale == w["scale"] and mo.center == w["center"]
        state = random.getstate(), np.random.get_state()   # (the fixture's probes left the generators where they were)
        assert random.random() == b["next_random"] and float(np.random.random()) == b["next_np_random"]
        random.setstate(state[0])
        np.random.set_state(state[1])


def test_the_packed_record_is_the_headers(data):
    from yolov3_amd import augment

    M = np.array([[1.25, -0.5, 3.0], [0.25, 0.75, -7.0], [0, 0, 1]], dtype=np.float64)
    M2 = np.array([[1.0, 0, -32], [0, 1, -32], [0, 0, 1]], dtype=np.float64)
    luts = np.stack([np.arange(256) % 180, 255 - np.arange(256), np.arange(256)]).astype(np.uint8)
    a = augment.Mosaic([5, 0, 7, 5], [(10, 20, 40, 50, 1, 2, 31, 32), (40, 0, 88, 50, 0, 14, 48, 64), (0, 50, 40, 91, 24, 0, 64, 41), (40, 50, 101, 114, 0, 0, 61, 64)], M, 1.5, 128,
                       [(9, 18), (40, -14), (-24, 50), (40, 50)], (50, 40))
    b = augment.Mosaic([3], [(20, 0, 43, 64, 0, 0, 23, 64)], M2, 0.75, 64, [(20.5, 0.0)])
    rec = augment.pack_items([augment.Item(5, [a, b], 0.4375, luts, True, False, True), augment.Item(3, [b], None, None, False, True, False)])
    raw = rec.tobytes()
    assert len(raw) == 2 * 1360
    inv = struct.unpack_from("<6d", raw, 0)
    D = 1.0 / (1.25 * 0.75 - (-0.5) * 0.25)
    assert inv[0] == 0.75 * D and inv[1] == 0.5 * D and inv[3] == -0.25 * D and inv[4] == 1.25 * D
    assert inv[2] == -inv[0] * 3.0 - inv[1] * -7.0 and inv[5] == -inv[3] * 3.0 - inv[4] * -7.0
    assert struct.unpack_from("<6d", raw, 48) == (1.25, -0.5, 3.0, 0.25, 0.75, -7.0) and struct.unpack_from("<d4i", raw, 96) == (1.5, 4, 128, 1, 0)
    assert struct.unpack_from("<7i2fi", raw, 120) == (5, 10, 20, 40, 50, 9, 18, 9.0, 18.0, 0)
    assert struct.unpack_from("<7i2fi", raw, 120 + 3 * 40) == (5, 40, 50, 101, 114, 40, 50, 40.0, 50.0, 0)
    assert struct.unpack_from("<6d", raw, 280) == (1.0, 0.0, 32.0, 0.0, 1.0, 32.0) and struct.unpack_from("<d4i", raw, 280 + 96) == (0.75, 1, 64, 1, 0)
    assert struct.unpack_from("<7i2fi", raw, 280 + 120) == (3, 20, 0, 43, 64, 20, 0, 20.5, 0.0, 0)
    assert struct.unpack_from("<2d4i", raw, 560) == (0.4375, 0.5625, 2, 1, 0, 1) and raw[592 : 592 + 768] == luts.tobytes()
    second = raw[1360:]
    assert struct.unpack_from("<d4i", second, 96) == (0.75, 1, 64, 0, 0) and struct.unpack_from("<2d4i", second, 560) == (0.0, 0.0, 1, 0, 1, 0)
    assert second[280:560] == bytes(280) and second[592:] == bytes(768)   # no second mosaic, no tables
    assert augment.invert_affine(M) == ac.invert_affine(M)   # the module's inverse is the statement's


def _ds(data, hyp=None, **kw):
    from yolov3_amd import DeviceTrainDataset

    args = dict(img_size=ac.IMG_SIZE, batch_size=ac.BATCH, stride=ac.STRIDE, shapes0=ac.hw0(), paths=ac.paths(), device="cpu")
    args.update(kw)
    return DeviceTrainDataset(args.pop("images", data.images), args.pop("labels", data.labels), dict(ac.CASES["low"]["hyp"]) if hyp is None else hyp, **args)


def test_every_refusal_comes_before_any_upload(data, monkeypatch):
    from yolov3_amd import dataset

    def no_upload(*a, **k):
        raise AssertionError("an upload was attempted")

    monkeypatch.setattr(dataset, "_upload", no_upload)
    monkeypatch.setattr(dataset, "_upload_arena", no_upload)
    low = ac.CASES["low"]["hyp"]
    with pytest.raises(RuntimeError, match="no CPU / PyTorch fallback"):   # valid inputs, a CPU device
        _ds(data)
    with pytest.raises(ValueError, match="perspective.*warpPerspective is not built"):
        _ds(data, dict(low, perspective=0.001))
    with pytest.raises(ValueError, match="copy_paste"):
        _ds(data, dict(low, copy_paste=0.1))
    with pytest.raises(ValueError, match="polygon labels"):
        _ds(data, segments=[[]] * 11 + [[np.zeros((5, 2), dtype=np.float32)]])
    with pytest.raises(RuntimeError, match="no CPU"):   # empty segments are what a box-only dataset holds: accepted, the device is what is missing
        _ds(data, segments=[[]] * 12)
    with pytest.raises(ValueError, match="rect=True.*mosaic = augment and not rect"):
        _ds(data, rect=True)
    short = list(data.images)
    short[4] = np.zeros((40, 50, 3), dtype=np.uint8)
    with pytest.raises(ValueError, match=r"image images/000005.png is 40x50: its long side is not img_size = 64.*cv2.resize"):
        _ds(data, images=short)
    for bad in (63, 72, 8):
        with pytest.raises(ValueError, match=f"img_size = {bad} must be a multiple of 16"):
            _ds(data, img_size=bad)
    for key in ("mosaic", "mixup", "degrees", "translate", "scale", "shear", "perspective", "hsv_h", "hsv_s", "hsv_v", "flipud", "fliplr", "copy_paste"):
        with pytest.raises(KeyError, match=key):
            _ds(data, {k: v for k, v in low.items() if k != key})
    with pytest.raises(TypeError, match="float64"):   # the shared constructor's refusals still apply
        _ds(data, dtype=torch.float64)
    with pytest.raises(ValueError, match="12 images, but 11 label arrays"):
        _ds(data, labels=data.labels[:11])


def test_from_dataset_reads_the_reference_dataset_and_device_dataset_still_refuses_it(data):
    from yolov3_amd import DeviceDataset, DeviceTrainDataset

    ref = SimpleNamespace(ims=data.images, im_hw0=ac.hw0(), im_hw=ac.hw(), labels=data.labels, segments=[[]] * 12, im_files=ac.paths(), rect=False, img_size=64, stride=32,
                          augment=True, mosaic=True, hyp=dict(ac.CASES["low"]["hyp"]), indices=range(12))
    with pytest.raises(ValueError, match="augment"):
        DeviceDataset.from_dataset(ref, batch_size=4, device="cpu")
    with pytest.raises(RuntimeError, match="no CPU"):   # everything read and accepted: the device is what is missing
        DeviceTrainDataset.from_dataset(ref, batch_size=4, device="cpu")
    ref.hyp["perspective"] = 0.5
    with pytest.raises(ValueError, match="perspective"):
        DeviceTrainDataset.from_dataset(ref, batch_size=4, device="cpu")
    ref.hyp["perspective"], ref.rect = 0.0, True
    with pytest.raises(ValueError, match="rect=True"):
        DeviceTrainDataset.from_dataset(ref, batch_size=4, device="cpu")
    ref.rect, ref.augment = False, False
    with pytest.raises(ValueError, match="does not augment"):
        DeviceTrainDataset.from_dataset(ref, batch_size=4, device="cpu")
    ref.augment, ref.ims = True, [None] * 12
    with pytest.raises(ValueError, match='cache="ram"'):
        DeviceTrainDataset.from_dataset(ref, batch_size=4, device="cpu")


def test_cpu_tensors_are_refused():
    from yolov3_amd import ops

    z = torch.zeros(32 * 12, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="no CPU"):
        ops.augment_batch(z, z, 12, torch.zeros(4 * 1360, dtype=torch.uint8), 4, 64)
    with pytest.raises(RuntimeError, match="no CPU"):
        ops.augment_targets(torch.zeros(4, 5), torch.zeros(13, dtype=torch.int64), z, 12, torch.zeros(4 * 1360, dtype=torch.uint8), 4, 64, 4)


def test_golden_is_what_the_live_reference_computes(gold):
    from oracle import ref_shim

    if not ref_shim.available():
        pytest.skip("the reference tree is not readable here")
    sys.path.insert(0, str(ROOT / "tests" / "golden"))
    import tempfile

    import make_augment_golden as gen

    with tempfile.TemporaryDirectory() as tmp:
        gen.write_tree(Path(tmp))
        live = gen.run_case(gen.reference(), Path(tmp), "exact", gen.new_stats())
    g = gold["cases"]["exact"]
    assert live["indices"] == g["indices"] and len(live["batches"]) == len(g["batches"])
    for a, b in zip(live["batches"], g["batches"]):
        assert torch.equal(a["im"], b["im"]) and torch.equal(a["targets"], b["targets"]) and a["shapes"] == b["shapes"] and a["paths"] == b["paths"]
        assert a["next_random"] == b["next_random"] and a["next_np_random"] == b["next_np_random"]
        assert all(torch.equal(x["M"], y["M"]) and x["rects"] == y["rects"] for ia, ib in zip(a["items"], b["items"]) for x, y in zip(ia["mosaics"], ib["mosaics"]))
