"""CPU tests of the device-resident dataset (csrc/dataset.hip, yolov3_amd/dataset.py): the public surface, the C ABI's argument validation without a GPU, the host
layout (aspect-ratio order, batch shapes, letterbox's top / left, the `shapes` tuples) against the fixture of the unmodified reference
(tests/golden/make_dataset_golden.py), and every refusal of the constructor -- all of them raised before anything is uploaded, so none needs a device."""
import re
import sys
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests"))

import dataset_cases as dc  # noqa: E402

NEW_SYMBOLS = ["y3_dataset_batch", "y3_dataset_targets"]


@pytest.fixture(scope="module")
def lib():
    from yolov3_amd import _lib, build

    build.build(verbose=False)
    return _lib.lib()


@pytest.fixture(scope="module")
def gold(golden_dir):
    return torch.load(golden_dir / "dataset.pt", weights_only=True)   # data only


@pytest.fixture(scope="module")
def data():
    return SimpleNamespace(images=dc.make_images(), labels=dc.make_labels())


def test_public_names_import():
    import yolov3_amd
    from yolov3_amd import DeviceDataset, dataset, ops, rect_batch_shapes

    assert dataset.DeviceDataset is DeviceDataset and dataset.rect_batch_shapes is rect_batch_shapes
    assert callable(yolov3_amd.rect_batch_shapes) and callable(DeviceDataset.from_dataset) and callable(ops.dataset_batch) and callable(ops.dataset_targets)
    assert "DeviceDataset" in yolov3_amd.__doc__ and "rect_batch_shapes" in yolov3_amd.__doc__


def test_new_symbols_are_declared_bound_and_exported_at_abi_6(lib):
    from yolov3_amd import _lib

    header = (ROOT / "include" / "yolov3_hip.h").read_text()
    declared = set(re.findall(r"\b(y3_[a-z0-9_]+)\s*\(", header))
    assert set(NEW_SYMBOLS) <= declared and set(NEW_SYMBOLS) <= set(_lib.exported_symbols()) and declared == set(_lib.exported_symbols())
    assert "#define Y3_ABI_VERSION 6" in re.sub(r"[ \t]+", " ", header) and lib.y3_abi_version() == 6 == _lib.ABI_VERSION
    assert ("dataset.hip", ["-ffp-contract=off"]) in __import__("yolov3_amd.build", fromlist=["SOURCES"]).SOURCES
    assert all(s in (ROOT / "INTEGRATION.md").read_text() for s in NEW_SYMBOLS + ["DeviceDataset", "rect_batch_shapes"])
    source = (ROOT / "yolov3_amd" / "dataset.py").read_text()
    assert "_lib" not in source and "ctypes" not in source   # the module marshals no C call itself
    assert not re.search(r"\b(F\.pad|torch\.(stack|cat|flip|clamp|where|nn))\b", source)   # no torch compute stands in for a kernel
    from yolov3_amd import dataset

    assert dataset._RECORD.itemsize == 32 and "} y3_dataset_image;" in header   # the record the module packs is the header's


def test_new_exports_reject_bad_arguments_without_a_gpu(lib):
    P = 1 << 20   # a fake, aligned device address: validation never dereferences it
    U8, F16, F32 = 3, 0, 2

    def fails(status, *needles):
        msg = lib.y3_last_error()
        assert status != 0 and all(n in msg for n in needles), (status, msg)

    def batch(arena=P, arena_bytes=4096, images=P, n=8, indices=None, first=0, count=3, dst=P, dtype=U8, H=64, W=96):
        return lib.y3_dataset_batch(arena, arena_bytes, images, n, indices, first, count, dst, dtype, H, W, None)

    fails(batch(arena=None), b"y3_dataset_batch", b"null")
    fails(batch(images=None), b"y3_dataset_batch", b"null")
    fails(batch(dst=None), b"y3_dataset_batch", b"null")
    fails(batch(n=0), b"y3_dataset_batch", b"geometry")
    fails(batch(count=-1), b"y3_dataset_batch", b"geometry")
    fails(batch(H=0), b"y3_dataset_batch", b"geometry")
    fails(batch(W=4112), b"y3_dataset_batch", b"geometry")
    fails(batch(H=65536), b"y3_dataset_batch", b"geometry")
    fails(batch(W=72), b"y3_dataset_batch", b"72 is not a multiple of 16")
    fails(batch(first=6), b"y3_dataset_batch", b"images 6 .. 8 lie outside the 8")
    fails(batch(first=-1), b"y3_dataset_batch", b"lie outside")
    fails(batch(indices=P + 4), b"y3_dataset_batch", b"8-byte aligned")
    fails(batch(images=P + 4), b"y3_dataset_batch", b"8-byte aligned")
    fails(batch(arena_bytes=4098), b"y3_dataset_batch", b"multiple of 4")
    fails(batch(arena_bytes=0), b"y3_dataset_batch", b"multiple of 4")
    fails(batch(arena=P + 8), b"y3_dataset_batch", b"16-byte aligned")
    fails(batch(dst=P + 8, dtype=F16), b"y3_dataset_batch", b"16-byte aligned")
    fails(batch(dtype=7), b"y3_dataset_batch", b"unsupported output dtype 7")
    fails(batch(count=1024, n=2048, H=65535, dtype=F32), b"y3_dataset_batch", b"too large")
    assert batch(count=0) == 0   # an empty batch launches nothing

    def targets(labels=P, offsets=P, images=P, n=8, indices=None, first=0, count=3, H=64, W=96, out=P, rows=5, out_offsets=P):
        return lib.y3_dataset_targets(labels, offsets, images, n, indices, first, count, H, W, out, rows, out_offsets, None)

    fails(targets(offsets=None), b"y3_dataset_targets", b"null")
    fails(targets(out_offsets=None), b"y3_dataset_targets", b"null")
    fails(targets(labels=None), b"y3_dataset_targets", b"null")
    fails(targets(out=None), b"y3_dataset_targets", b"null")
    fails(targets(images=None), b"y3_dataset_targets", b"null")
    fails(targets(n=-2), b"y3_dataset_targets", b"geometry")
    fails(targets(W=100), b"y3_dataset_targets", b"100 is not a multiple of 16")
    fails(targets(first=7), b"y3_dataset_targets", b"lie outside")
    fails(targets(count=1025, n=4096), b"y3_dataset_targets", b"1025 images unsupported")
    fails(targets(rows=-1), b"y3_dataset_targets", b"geometry")
    fails(targets(rows=1 << 31), b"y3_dataset_targets", b"geometry")
    fails(targets(offsets=P + 4), b"y3_dataset_targets", b"aligned")
    fails(targets(out_offsets=P + 4), b"y3_dataset_targets", b"aligned")
    fails(targets(labels=P + 2), b"y3_dataset_targets", b"aligned")
    fails(targets(indices=P + 4), b"y3_dataset_targets", b"aligned")


def test_case_builders_reproduce_the_golden(gold, data):
    assert list(gold["cases"]) == list(dc.CASES) and abs(dc.checksum(data.images, data.labels) - gold["checksum"]) < 1e-6
    assert [im.shape for im in data.images] == [(h, w, 3) for h, w in dc.hw()] and all(im.dtype == np.uint8 for im in data.images)
    assert all(lb.dtype == np.float32 and lb.shape[1] == 5 for lb in data.labels) and [len(lb) for lb in data.labels] == [4, 6, 0, 2, 0, 3, 1, 0]
    # the shapes the issue asks for occur: wide-only, mixed and tall-only batch shapes, widths 64 and 96, a last partial batch, a batch without labels
    g = gold["cases"]["rect_pad05"]
    assert g["batch_shapes"].tolist() == [[64, 96], [96, 96], [96, 64]] and gold["cases"]["rect_pad00"]["batch_shapes"].tolist() == [[32, 64], [64, 64], [64, 64]]
    assert [len(b["paths"]) for b in g["batches"]] == [3, 3, 2] and [len(b["targets"]) for b in g["batches"]] == [3, 13, 0]
    assert g["order"].tolist() == dc.RECT_ORDER and sorted(dc.CASES["square_perm"]["indices"]) == list(range(8)) != dc.CASES["square_perm"]["indices"]
    pads = [s[1][1] for c in gold["cases"].values() for b in c["batches"] for s in b["shapes"]]
    assert (17.5, 29.5) in pads and (1.5, 13.5) in pads and (20.5, 0.0) in pads and (0.0, 0.0) in pads   # halves that differ, and no border at all
    sq = gold["cases"]["square"]["batches"][0]["targets"]   # E in a 64 x 64 batch: the clip at 64 - 1e-3 acted, and a zero-area box stayed one
    e = sq[sq[:, 0] == 1]
    assert torch.equal(e[0, 2:], torch.tensor([np.float32(((np.float32(32.0) + np.float32(64 - 1e-3)) / 2) / 64), 0.5, np.float32((np.float32(64 - 1e-3) - 32) / 64), 0.5]))
    assert (e[3, 4:] == 0).all() and (e[4, 4:] == 0).all() and float(e[4, 2]) == float(np.float32(np.float32(64 - 1e-3) / 64))
    assert (gold["cases"]["rect_single_cls"]["batches"][1]["targets"][:, 1] == 0).all() and (gold["cases"]["rect_pad05"]["batches"][1]["targets"][:, 1] != 0).any()


def test_rect_batch_shapes_is_the_reference_layout(gold):
    from yolov3_amd import rect_batch_shapes

    wh = [(w0, h0) for h0, w0 in dc.hw0()]
    for case in ("rect_pad05", "rect_pad00"):
        g = gold["cases"][case]
        order, batch, shapes = rect_batch_shapes(np.array(wh), dc.IMG_SIZE, dc.BATCH, dc.STRIDE, dc.CASES[case]["pad"])
        assert order.tolist() == g["order"].tolist() and batch.tolist() == g["batch"].tolist() and shapes.tolist() == g["batch_shapes"].tolist()
    order, batch, shapes = rect_batch_shapes(wh, 640, 32, 32, 0.5)   # one batch, mixed: the square shape plus the pad
    assert sorted(order.tolist()) == list(range(8)) and batch.tolist() == [0] * 8 and shapes.tolist() == [[672, 672]]
    with pytest.raises(ValueError, match=r"\(n, 2\)"):
        rect_batch_shapes(np.zeros((0, 2)), 64, 3, 32, 0.5)


@pytest.mark.parametrize("case", list(dc.CASES))
def test_layout_top_left_and_shapes_equal_the_fixture(gold, data, case):
    from yolov3_amd import dataset

    c, g = dc.CASES[case], gold["cases"][case]
    lay = dataset.layout(dc.hw(), dc.hw0(), dc.IMG_SIZE, dc.BATCH, dc.STRIDE, c["pad"], c["rect"], dc.paths())
    assert lay.order.tolist() == g["order"].tolist() and lay.batch.tolist() == g["batch"].tolist()
    assert [dc.paths()[i] for i in lay.order] == g["paths"]
    if c["rect"]:
        assert lay.batch_shapes.tolist() == g["batch_shapes"].tolist()
    epoch = c["indices"] or list(range(len(dc.IMAGES)))
    for k, b in enumerate(g["batches"]):
        which = epoch[k * dc.BATCH : (k + 1) * dc.BATCH]
        got = tuple(lay.shapes[j] for j in which)
        assert got == b["shapes"] and all(type(x) is type(y) for s, t in zip(got, b["shapes"]) for x, y in zip(s[0] + s[1][0] + s[1][1], t[0] + t[1][0] + t[1][1]))
        want = dc.expected_images(gold, case, k)
        for slot, j in enumerate(which):   # top / left: where the fixture's letterboxed image holds the cached one (RGB planes of a BGR source)
            im = data.images[lay.order[j]]
            h, w = im.shape[:2]
            t, l = int(lay.top[j]), int(lay.left[j])
            (dw, dh) = b["shapes"][slot][1][1]
            assert (t, l) == (round(dh - 0.1), round(dw - 0.1))
            assert np.array_equal(want[slot, :, t : t + h, l : l + w].numpy(), im.transpose(2, 0, 1)[::-1])
            border = want[slot].clone()
            border[:, t : t + h, l : l + w] = 114
            assert (border == 114).all()


def _ds(data, **kw):
    from yolov3_amd import DeviceDataset

    args = dict(img_size=dc.IMG_SIZE, batch_size=dc.BATCH, stride=dc.STRIDE, pad=0.5, rect=True, shapes0=dc.hw0(), paths=dc.paths(), device="cpu")
    args.update(kw)
    return DeviceDataset(args.pop("images", data.images), args.pop("labels", data.labels), **args)


def test_every_refusal_comes_before_any_upload(data, monkeypatch):
    from yolov3_amd import DeviceDataset, dataset

    def no_upload(*a, **k):
        raise AssertionError("an upload was attempted")

    monkeypatch.setattr(dataset, "_upload", no_upload)
    monkeypatch.setattr(dataset, "_upload_arena", no_upload)
    with pytest.raises(RuntimeError, match="no CPU / PyTorch fallback"):   # valid inputs, a CPU device
        _ds(data)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU / PyTorch fallback"):
            _ds(data, device="cuda")
        with pytest.raises(RuntimeError, match="no CPU / PyTorch fallback"):
            _ds(data, device=None)
    bad = list(data.images)
    bad[2] = bad[2].astype(np.float32)
    with pytest.raises(TypeError, match=r"image images/000003.png is float32 \(64, 41, 3\), not a uint8 \(h, w, 3\) array"):
        _ds(data, images=bad)
    bad[2] = data.images[2][:, :, 0]
    with pytest.raises(TypeError, match=r"not a uint8 \(h, w, 3\) array"):
        _ds(data, images=bad)
    bad[2] = torch.from_numpy(data.images[2])
    with pytest.raises(TypeError, match="image images/000003.png is Tensor"):
        _ds(data, images=bad)
    with pytest.raises(TypeError, match="float64"):
        _ds(data, dtype=torch.float64)
    tall = list(data.images)
    tall[6] = np.zeros((40, 64, 3), dtype=np.uint8)   # A's batch is 32 x 64 with pad 0: 40 rows need a resize
    with pytest.raises(ValueError, match=r"image images/000007.png \(40x64\) does not fit its batch shape 32x64.*cv2.resize"):
        _ds(data, images=tall, pad=0.0)
    wide = list(data.images)
    wide[1] = np.zeros((64, 70, 3), dtype=np.uint8)
    with pytest.raises(ValueError, match=r"images/000002.png \(64x70\) does not fit its batch shape 64x64"):
        _ds(data, images=wide, rect=False)
    lb = list(data.labels)
    lb[3] = np.zeros((2, 6), dtype=np.float32)
    with pytest.raises(ValueError, match=r"labels of image images/000004.png have shape \(2, 6\), not \(m, 5\)"):
        _ds(data, labels=lb)
    lb[3] = np.zeros(5, dtype=np.float32)
    with pytest.raises(ValueError, match=r"not \(m, 5\)"):
        _ds(data, labels=lb)
    with pytest.raises(ValueError, match="8 images, but 7 label arrays"):
        _ds(data, labels=data.labels[:7])
    with pytest.raises(ValueError, match="no images"):
        DeviceDataset([], [], device="cpu")
    with pytest.raises(ValueError, match="batch width 72 is not a multiple of 16"):
        _ds(data, images=[np.zeros((8, 8, 3), dtype=np.uint8)] * 8, rect=False, img_size=72)
    with pytest.raises(ValueError, match="batch_size"):
        _ds(data, batch_size=0)


def test_set_indices_is_refused_on_a_rect_set_and_checks_its_indices(data):
    from yolov3_amd import DeviceDataset

    def shell(rect):   # a set as the constructor leaves it, minus the device buffers
        ds = object.__new__(DeviceDataset)
        ds.rect, ds.n, ds.batch_size, ds.device, ds._perm, ds._perm_dev = rect, 8, 3, torch.device("cpu"), None, None
        return ds

    with pytest.raises(ValueError, match="rect=True set keeps its aspect-ratio order"):
        shell(True).set_indices([0, 1, 2])
    for bad in ([0, 8], [-1], [], [0.5, 1.0]):
        with pytest.raises(ValueError, match=r"image indices in \[0, 8\)"):
            shell(False).set_indices(bad)
    ds = shell(False)
    assert len(ds) == 3 and ds.batch_images(2) == [6, 7]
    ds.set_indices(None)
    assert ds._perm is None


def test_from_dataset_refuses_a_dataset_without_a_ram_cache(data):
    from yolov3_amd import DeviceDataset

    ref = SimpleNamespace(ims=[None] * 8, im_hw0=dc.hw0(), im_hw=dc.hw(), labels=data.labels, im_files=dc.paths(), rect=True, img_size=64, stride=32, augment=False)
    with pytest.raises(ValueError, match='cache="ram"'):
        DeviceDataset.from_dataset(ref, batch_size=3, device="cpu")
    ref.ims, ref.augment = data.images, True
    with pytest.raises(ValueError, match="augment"):
        DeviceDataset.from_dataset(ref, batch_size=3, device="cpu")
    ref.augment, ref.im_hw = False, [(1, 1)] * 8
    with pytest.raises(ValueError, match="im_hw"):
        DeviceDataset.from_dataset(ref, batch_size=3, device="cpu")
    ref.im_hw, ref.batch, ref.batch_shapes = dc.hw(), np.array([0, 0, 0, 0, 1, 1, 1, 1]), np.array([[64, 96], [96, 96]])   # built for batches of 4
    with pytest.raises(ValueError, match="batches of 3"):
        DeviceDataset.from_dataset(ref, batch_size=3, device="cpu")


def test_cpu_tensors_are_refused():
    from yolov3_amd import ops

    z = torch.zeros(256, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="no CPU"):
        ops.dataset_batch(z, z, 8, None, 0, 3, 64, 64)
    with pytest.raises(RuntimeError, match="no CPU"):
        ops.dataset_targets(torch.zeros(4, 5), torch.zeros(9, dtype=torch.int64), z, 8, None, 0, 3, 64, 64, 4)


@pytest.mark.parametrize("case", ["rect_pad05", "square_perm"])
def test_golden_is_what_the_live_reference_computes(gold, case):
    from oracle import ref_shim

    if not ref_shim.available():
        pytest.skip("the reference tree is not readable here")
    sys.path.insert(0, str(ROOT / "tests" / "golden"))
    import tempfile

    import make_dataset_golden as gen

    stored = {}
    with tempfile.TemporaryDirectory() as tmp:
        gen.write_tree(Path(tmp))
        d = gen.reference()
        if case in dc.IMAGES_OF:
            stored[dc.IMAGES_OF[case]] = gold["cases"][dc.IMAGES_OF[case]]
        live = gen.run_case(d, Path(tmp), case, stored)
    g = gold["cases"][case]
    assert live["order"].tolist() == g["order"].tolist() and live["paths"] == g["paths"]
    for a, b in zip(live["batches"], g["batches"]):
        assert torch.equal(a["targets"], b["targets"]) and a["shapes"] == b["shapes"] and a["paths"] == b["paths"]
        assert torch.equal(a["im"], b["im"]) if "im" in b else a["im_from"] == b["im_from"]
