"""GPU tests of the device-resident dataset (csrc/dataset.hip through yolov3_amd/dataset.py) against tests/golden/dataset.pt: the batches the unmodified reference's
LoadImagesAndLabels.__getitem__ and collate_fn produce for the same cached images (tests/golden/make_dataset_golden.py).  Images must be equal byte for byte, targets
bit for bit, paths and shapes equal; the floating outputs are compared with `im_u8.to(dtype) / 255` of the fixture's uint8 batch (IEEE division, formed on the host).
Shapes: tests/dataset_cases.py -- 8 images, batches of 3, 64 px: every alignment of a source row, every border form, several blocks per launch."""
import sys
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests"))

import dataset_cases as dc  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def gold(golden_dir):
    return torch.load(golden_dir / "dataset.pt", weights_only=True)   # data only


@pytest.fixture(scope="module")
def data():
    return SimpleNamespace(images=dc.make_images(), labels=dc.make_labels())


def _build(data, case, dev, dtype=torch.uint8):
    from yolov3_amd import DeviceDataset

    c = dc.CASES[case]
    ds = DeviceDataset(data.images, data.labels, img_size=dc.IMG_SIZE, batch_size=dc.BATCH, stride=dc.STRIDE, pad=c["pad"], rect=c["rect"], shapes0=dc.hw0(), paths=dc.paths(),
                       single_cls=c["single_cls"], device=dev, dtype=dtype)
    if c["indices"] is not None:
        ds.set_indices(c["indices"])
    return ds


@pytest.fixture(scope="module")
def sets(data, dev):
    """every case once, uint8 (left unchanged by the tests)"""
    return {case: _build(data, case, dev) for case in dc.CASES}


def _same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    return a.shape == b.shape and a.dtype == b.dtype == torch.float32 and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _assert_batches(ds, gold, case, dev):
    g = gold["cases"][case]
    assert len(ds) == len(g["batches"])
    n = 0
    for k, ((im, targets, paths, shapes), want) in enumerate(zip(ds, g["batches"])):
        assert im.device == dev == targets.device and im.dtype == torch.uint8 and im.is_contiguous()
        assert torch.equal(im.cpu(), dc.expected_images(gold, case, k)), f"{case}: images of batch {k}"
        assert _same_bits(targets.cpu(), want["targets"]), f"{case}: targets of batch {k}\n{targets.cpu()}\n{want['targets']}"
        assert isinstance(paths, tuple) and list(paths) == want["paths"] and isinstance(shapes, tuple) and shapes == want["shapes"]
        n += 1
    assert n == len(g["batches"])


@pytest.mark.parametrize("case", list(dc.CASES))
def test_every_batch_is_the_reference_loaders(sets, gold, case, dev):
    ds = sets[case]
    if dc.CASES[case]["rect"]:
        assert ds.order.tolist() == gold["cases"][case]["order"].tolist() and ds.batch_shapes.tolist() == gold["cases"][case]["batch_shapes"].tolist()
    _assert_batches(ds, gold, case, dev)
    _assert_batches(ds, gold, case, dev)   # a second epoch gives identical batches


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float32])
@pytest.mark.parametrize("case", ["rect_pad05", "rect_pad00", "square_perm"])
def test_floating_batches_are_the_uint8_batch_divided_by_255(data, gold, case, dtype, dev):
    ds = _build(data, case, dev, dtype)
    for k, (im, targets, _, _) in enumerate(ds):
        want = dc.expected_images(gold, case, k).to(dtype) / 255
        assert im.dtype == dtype and torch.equal(im.cpu(), want), f"{case} {dtype}: batch {k}"
        assert _same_bits(targets.cpu(), gold["cases"][case]["batches"][k]["targets"])


def test_offsets_of_the_targets(sets, gold, dev):
    from yolov3_amd import ops

    ds = sets["rect_pad05"]
    for k, want in enumerate(gold["cases"]["rect_pad05"]["batches"]):
        which = ds.batch_images(k)
        H, W = (int(v) for v in ds.batch_shapes[k])
        targets, offsets = ops.dataset_targets(ds._labels, ds._label_offsets, ds._records, ds.n, None, which[0], len(which), H, W, len(want["targets"]))
        counts = torch.bincount(want["targets"][:, 0].long(), minlength=len(which))
        assert offsets.dtype == torch.int64 and offsets.cpu().tolist() == [0] + torch.cumsum(counts, 0).tolist()
        assert _same_bits(targets.cpu(), want["targets"])


def test_from_dataset_adopts_the_order_of_a_reference_dataset(data, gold, dev):
    from yolov3_amd import DeviceDataset

    for case in ("rect_pad00", "square_perm", "rect_single_cls"):
        c, g = dc.CASES[case], gold["cases"][case]
        order = g["order"].tolist()
        labels = [data.labels[i].copy() for i in order]
        ref = SimpleNamespace(ims=[data.images[i] for i in order], im_hw0=[dc.hw0()[i] for i in order], im_hw=[dc.hw()[i] for i in order], labels=labels,
                              im_files=list(g["paths"]), rect=c["rect"], img_size=dc.IMG_SIZE, stride=dc.STRIDE, augment=False, batch=g["batch"].numpy(),
                              indices=c["indices"] if c["indices"] is not None else range(len(order)))
        if c["rect"]:
            ref.batch_shapes = g["batch_shapes"].numpy()
        ds = DeviceDataset.from_dataset(ref, batch_size=dc.BATCH, device=dev, single_cls=c["single_cls"])
        assert ds.order.tolist() == list(range(len(order))) and ds.paths == g["paths"]
        _assert_batches(ds, gold, case, dev)
        assert all(np.array_equal(a, data.labels[i]) for a, i in zip(labels, order))   # single_cls did not reach the caller's arrays


def test_set_indices_changes_the_epoch_and_none_restores_it(data, gold, dev):
    ds = _build(data, "square", dev)
    _assert_batches(ds, gold, "square", dev)
    ds.set_indices(dc.CASES["square_perm"]["indices"])
    _assert_batches(ds, gold, "square_perm", dev)
    ds.set_indices(None)
    _assert_batches(ds, gold, "square", dev)
    ds.set_indices([1, 1, 1, 1])   # a weighted draw repeats images: one full batch and a partial one of the same image
    (a, ta, pa, _), (b, tb, pb, _) = list(ds)
    want = gold["cases"]["square"]["batches"][0]
    assert a.shape[0] == 3 and b.shape[0] == 1 and all(torch.equal(x.cpu(), want["im"][1]) for x in (*a, *b)) and pa == (dc.paths()[1],) * 3 and pb == (dc.paths()[1],)
    e = want["targets"][want["targets"][:, 0] == 1][:, 1:]
    assert torch.equal(ta.cpu()[:, 1:], e.repeat(3, 1)) and ta.cpu()[:, 0].tolist() == [0.0] * 6 + [1.0] * 6 + [2.0] * 6 and torch.equal(tb.cpu()[:, 1:], e)


@pytest.mark.parametrize("dtype", [torch.uint8, torch.float16, torch.float32])
@pytest.mark.parametrize("case,k", [("rect_pad00", 1), ("rect_pad05", 0)])   # W = 64 and W = 96
def test_a_sliced_output_keeps_the_bytes_around_it(sets, gold, case, k, dtype, dev):
    from yolov3_amd import ops

    ds = sets[case]
    which = ds.batch_images(k)
    H, W = (int(v) for v in ds.batch_shapes[k])
    assert W == (64 if case == "rect_pad00" else 96)
    want = dc.expected_images(gold, case, k)
    want = want if dtype == torch.uint8 else want.to(dtype) / 255
    guard = 77 if dtype == torch.uint8 else -3.0
    # a slice of a larger batch: one image of guard values before and behind
    big = torch.full((len(which) + 2, 3, H, W), guard, dtype=dtype, device=dev)
    out = ops.dataset_batch(ds._arena, ds._records, ds.n, None, which[0], len(which), H, W, dtype, out=big[1:-1])
    assert out.data_ptr() == big[1].data_ptr() and torch.equal(big[1:-1].cpu(), want) and (big[0] == guard).all() and (big[-1] == guard).all()
    # an offset into a flat buffer: 16 bytes of guard before, 16 behind
    per = 16 // big.element_size()
    flat = torch.full((want.numel() + 2 * per,), guard, dtype=dtype, device=dev)
    ops.dataset_batch(ds._arena, ds._records, ds.n, None, which[0], len(which), H, W, dtype, out=flat[per:-per].view(want.shape))
    assert torch.equal(flat[per:-per].view(want.shape).cpu(), want) and (flat[:per] == guard).all() and (flat[-per:] == guard).all()
    with pytest.raises(Exception, match="16-byte aligned"):   # refused, not written
        ops.dataset_batch(ds._arena, ds._records, ds.n, None, which[0], len(which), H, W, dtype, out=flat[1 : 1 + want.numel()].view(want.shape))
    with pytest.raises(TypeError, match="contiguous"):
        ops.dataset_batch(ds._arena, ds._records, ds.n, None, which[0], len(which), H, W, dtype, out=big[1:-1, :, :, : W // 2])


def test_indices_outside_the_set_give_border_images_and_no_targets(sets, dev):
    """the kernel's own bound: the wrappers refuse such a batch, the library writes border and reads nothing"""
    from yolov3_amd import ops

    ds = sets["square"]
    idx = torch.tensor([ds.n, -1, 1], dtype=torch.int64, device=dev)
    im = ops.dataset_batch(ds._arena, ds._records, ds.n, idx, 0, 3, 64, 64)
    targets, offsets = ops.dataset_targets(ds._labels, ds._label_offsets, ds._records, ds.n, idx, 0, 3, 64, 64, 6)
    assert (im[:2] == 114).all() and not (im[2] == 114).all() and offsets.cpu().tolist() == [0, 0, 0, 6] and (targets[:, 0] == 2).all()


def _tiny(dev, golden_dir):
    from yolov3_amd import DetectMultiBackend, compat

    m = DetectMultiBackend(str(golden_dir / "ref_tiny_w025_fp16.pt"), device=dev, fp16=False)   # yolov3-tiny at width 0.25, pickled by the unmodified reference
    compat.uninstall_aliases()
    return m


@pytest.mark.parametrize("dtype", [torch.uint8, torch.float16])
def test_run_batches_over_the_set_is_run_batches_over_the_host_batches(data, gold, golden_dir, dtype, dev, tmp_path):
    from yolov3_amd import run_batches

    m = _tiny(dev, golden_dir)
    case = "rect_pad05"
    host = [(dc.expected_images(gold, case, k), b["targets"], b["paths"], b["shapes"]) for k, b in enumerate(gold["cases"][case]["batches"])]
    ds = _build(data, case, dev, dtype)
    kw = dict(nc=80, conf_thres=1e-4, half=dtype == torch.float16, save_json=True)   # (the random-weight checkpoint scores obj x cls around 2e-4)
    with torch.no_grad():
        want = run_batches(m, host, save_dir=tmp_path / "host", **kw)
        got = run_batches(m, ds, save_dir=tmp_path / "device", **kw)
    assert got[0] == want[0] and np.array_equal(got[1], want[1])
    a, b = got[2], want[2]
    assert a.n == b.n > 0 and np.array_equal(a.nt, b.nt) and a.nt.sum() == 16
    assert torch.equal(a._conf[: a.n], b._conf[: b.n]) and torch.equal(a._cls[: a.n], b._cls[: b.n]) and torch.equal(a._mask[: a.n], b._mask[: b.n])
    assert all(np.array_equal(x, y) for x, y in zip(a.compute(), b.compute()))
    assert (tmp_path / "device" / "predictions.json").read_bytes() == (tmp_path / "host" / "predictions.json").read_bytes()
