"""GPU tests of the host-resident image store (store="host": csrc/dataset_stage.hip through yolov3_amd/dataset.py and augment.py).  The three datasets keep their images in
pinned host memory and stage each batch's into a device ring; the batches must be what the resident sets yield, which is what the unmodified reference yields: the same
goldens as tests/test_gpu_augment*.py and test_gpu_dataset.py, images equal byte for byte, targets bit for bit, paths and shapes equal, no tolerance anywhere, once with
prefetch=0 and once with prefetch=1.  Shapes: the 12-image sets with a long side of 64 in batches of 4 (three or four batches over two ring halves: every half is
overwritten while the epoch runs) and the 8-image set of tests/dataset_cases.py, whose first image is 37 x 61 -- a size that is no multiple of 16.
The export alone runs on a synthetic arena whose images straddle the chunk size."""
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
import dataset_cases as dc  # noqa: E402

pytestmark = pytest.mark.gpu
CP_CASES = cpc.cases()
CANARY = 0xA5


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def golds(golden_dir):
    return {name: torch.load(golden_dir / f"{name}.pt", weights_only=True) for name in ("augment", "augment_polygons", "augment_copy_paste", "augment_rect", "dataset")}   # data only


@pytest.fixture(scope="module")
def poly():
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


def _bits(a: torch.Tensor) -> torch.Tensor:
    assert a.dtype == torch.float32
    return a.contiguous().view(torch.int32)


def _epoch(ds, seed=None):
    if seed is not None:
        _seed(seed)
    return [(im.cpu(), targets.cpu(), paths, shapes) for im, targets, paths, shapes in ds]


def _same_epochs(a, b):
    return len(a) == len(b) and all(torch.equal(x[0], y[0]) and x[1].shape == y[1].shape and torch.equal(_bits(x[1]), _bits(y[1])) and x[2:] == y[2:] for x, y in zip(a, b))


def _assert_store(ds, per_item, images):
    """the set lives in pinned host memory; the device holds two halves sized for the worst batch and nothing of the full size"""
    slots = np.sort(np.array([-(-im.nbytes // 16) * 16 for im in images], dtype=np.int64))[::-1]
    half = int(slots[: min(ds.n, per_item * ds.batch_size)].sum())
    assert ds.store == "host" and ds._arena is None and ds._records is None
    assert ds.host_bytes == int(slots.sum()) == ds._store.arena.numel() and ds._store.arena.is_pinned() and not ds._store.arena.is_cuda
    assert ds.ring_bytes == 2 * half == ds._store.ring.numel() and ds._store.ring.is_cuda and all(r.numel() == 32 * ds.n for r in ds._store.records)


def _train(images, labels, c, dev, prefetch, **kw):
    from yolov3_amd import DeviceTrainDataset

    ds = DeviceTrainDataset(images, labels, c["hyp"], img_size=ac.IMG_SIZE, batch_size=ac.BATCH, stride=ac.STRIDE, shapes0=ac.hw0(), paths=ac.paths(), device=dev,
                            dtype=getattr(torch, c.get("dtype", "uint8")), **({} if prefetch is None else dict(store="host", prefetch=prefetch)), **kw)
    if c["indices"] is not None:
        ds.set_indices(c["indices"])
    return ds


@pytest.mark.parametrize("prefetch", [0, 1])
@pytest.mark.parametrize("case", list(ac.CASES))
def test_the_train_set_in_host_memory_yields_the_reference_loaders_batches(golds, case, prefetch, dev):
    c, gold = ac.CASES[case], golds["augment"]
    ds = _train(ac.make_images(), ac.make_labels(), c, dev, prefetch)
    assert ds.prefetch == prefetch
    _assert_store(ds, 8 if c["hyp"]["mixup"] > 0 else 4, ac.make_images())
    got = _epoch(ds, c["seed"])
    g = gold["cases"][case]["batches"]
    assert len(got) == len(g) >= 3   # more batches than ring halves
    for k, ((im, targets, paths, shapes), want) in enumerate(zip(got, g)):
        u8 = ac.expected_images(gold, case, k)
        w = u8 if c["dtype"] == "uint8" else u8.to(getattr(torch, c["dtype"])) / 255
        assert im.dtype == w.dtype and torch.equal(im, w), f"{case}: images of batch {k}: {int((im != w).sum())} elements differ"
        assert targets.shape == want["targets"].shape and torch.equal(_bits(targets), _bits(want["targets"])), f"{case}: targets of batch {k}"
        assert isinstance(paths, tuple) and list(paths) == want["paths"] and isinstance(shapes, tuple) and shapes == want["shapes"]
    assert (random.random(), float(np.random.random())) == (g[-1]["next_random"], g[-1]["next_np_random"])   # the generators end where the reference's end


def test_a_letterbox_only_set_sizes_its_ring_for_one_image_per_item(dev):
    from yolov3_amd import DeviceTrainDataset

    ds = DeviceTrainDataset(ac.make_images(), ac.make_labels(), ac.CASES["low"]["hyp"], img_size=ac.IMG_SIZE, batch_size=ac.BATCH, stride=ac.STRIDE, device=dev, mosaic=False,
                            store="host")
    assert ds.prefetch == 1   # the default under store="host"
    _assert_store(ds, 1, ac.make_images())
    resident = DeviceTrainDataset(ac.make_images(), ac.make_labels(), ac.CASES["low"]["hyp"], img_size=ac.IMG_SIZE, batch_size=ac.BATCH, stride=ac.STRIDE, device=dev, mosaic=False)
    assert (resident.store, resident.prefetch, resident.host_bytes, resident.ring_bytes, resident._store) == ("device", 0, 0, 0, None)
    assert _same_epochs(_epoch(ds, 3), _epoch(resident, 3))


@pytest.mark.parametrize("prefetch", [0, 1])
@pytest.mark.parametrize("case", list(apc.CASES))
def test_polygon_labels_over_the_host_store(poly, golds, case, prefetch, dev):
    """targets and paths against the reference's golden; the fixture holds no images: they are those of the resident set, which tests/test_gpu_augment_polygons.py pins"""
    c, g = apc.CASES[case], golds["augment_polygons"]["cases"][case]["batches"]
    ds = _train(poly.images, poly.labels, c, dev, prefetch, segments=poly.segments)
    resident = _train(poly.images, poly.labels, c, dev, None, segments=poly.segments)
    got, want_im = _epoch(ds, c["seed"]), _epoch(resident, c["seed"])
    assert len(got) == len(g) == len(want_im)
    for k, ((im, targets, paths, shapes), want, (rim, rt, rp, rs)) in enumerate(zip(got, g, want_im)):
        assert targets.shape == want["targets"].shape and torch.equal(_bits(targets), _bits(want["targets"])), f"{case}: targets of batch {k}"
        assert list(paths) == want["paths"] and torch.equal(im, rim) and shapes == rs, f"{case}: batch {k}"


@pytest.mark.parametrize("prefetch", [0, 1])
@pytest.mark.parametrize("case", list(CP_CASES))
def test_copy_paste_over_the_host_store(poly, golds, case, prefetch, dev):
    """the candidates of a pasting batch ride between its records and the stage's jobs in one pinned copy: targets bit for bit, the images by the reference's checksum"""
    c, g = CP_CASES[case], golds["augment_copy_paste"]["cases"][case]["batches"]
    ds = _train(poly.images, poly.labels, c, dev, prefetch, segments=poly.segments, copy_paste=True)
    got = _epoch(ds, c["seed"])
    assert len(got) == len(g)
    for k, ((im, targets, paths, shapes), want) in enumerate(zip(got, g)):
        assert im.dtype == torch.uint8 and cpc.crc(im.numpy()) == want["im_crc"], f"{case}: image of batch {k}"
        assert targets.shape == want["targets"].shape and torch.equal(_bits(targets), _bits(want["targets"])), f"{case}: targets of batch {k}"
        assert list(paths) == want["paths"]
    assert (random.random(), float(np.random.random())) == (g[-1]["next_random"], g[-1]["next_np_random"])


@pytest.mark.parametrize("prefetch", [0, 1])
@pytest.mark.parametrize("case", list(arc.CASES))
def test_the_rect_train_set_in_host_memory(golds, case, prefetch, dev):
    from yolov3_amd import DeviceRectTrainDataset

    c, gold = arc.CASES[case], golds["augment_rect"]
    ds = DeviceRectTrainDataset(ac.make_images(), ac.make_labels(), c["hyp"], img_size=arc.IMG_SIZE, batch_size=arc.BATCH, stride=arc.STRIDE, shapes0=ac.hw0(), paths=ac.paths(),
                                device=dev, dtype=getattr(torch, c["dtype"]), store="host", prefetch=prefetch)
    _assert_store(ds, 1, ac.make_images())
    got = _epoch(ds, c["seed"])
    g = gold["cases"][case]["batches"]
    assert len(got) == len(g) == 3
    for k, ((im, targets, paths, shapes), want) in enumerate(zip(got, g)):
        u8 = arc.expected_images(gold, case, k)
        w = u8 if c["dtype"] == "uint8" else u8.to(getattr(torch, c["dtype"])) / 255
        assert im.dtype == w.dtype and im.shape == (4, 3, *arc.BATCH_SHAPES[k]) and torch.equal(im, w), f"{case}: images of batch {k}"
        assert targets.shape == want["targets"].shape and torch.equal(_bits(targets), _bits(want["targets"])), f"{case}: targets of batch {k}"
        assert list(paths) == want["paths"] and shapes == want["shapes"]


def _val(case, dev, **kw):
    from yolov3_amd import DeviceDataset

    c = dc.CASES[case]
    ds = DeviceDataset(dc.make_images(), dc.make_labels(), img_size=dc.IMG_SIZE, batch_size=dc.BATCH, stride=dc.STRIDE, pad=c["pad"], rect=c["rect"], shapes0=dc.hw0(), paths=dc.paths(),
                       single_cls=c["single_cls"], device=dev, **kw)
    if c["indices"] is not None:
        ds.set_indices(c["indices"])
    return ds


@pytest.mark.parametrize("prefetch", [0, 1])
@pytest.mark.parametrize("case", list(dc.CASES))
def test_the_val_set_in_host_memory(golds, case, prefetch, dev):
    """rect and square, the square set with set_indices; the first image of this set is 37 x 61: its 6771 bytes end 13 bytes short of their slot"""
    gold = golds["dataset"]
    ds = _val(case, dev, store="host", prefetch=prefetch)
    _assert_store(ds, 1, dc.make_images())
    assert any(im.nbytes % 16 for im in dc.make_images())
    for _ in range(2):   # a second epoch starts on whichever half the first one ended
        got = _epoch(ds)
        g = gold["cases"][case]["batches"]
        assert len(got) == len(g) == len(ds)
        for k, ((im, targets, paths, shapes), want) in enumerate(zip(got, g)):
            assert im.dtype == torch.uint8 and torch.equal(im, dc.expected_images(gold, case, k)), f"{case}: images of batch {k}"
            assert targets.shape == want["targets"].shape and torch.equal(_bits(targets), _bits(want["targets"])), f"{case}: targets of batch {k}"
            assert isinstance(paths, tuple) and list(paths) == want["paths"] and isinstance(shapes, tuple) and shapes == want["shapes"]


def test_set_indices_with_a_repeating_draw_on_the_host_store(golds, dev):
    ds = _val("square", dev, store="host")
    ds.set_indices([1, 1, 1, 1])   # one full batch and a partial one of the same image: staged once per batch
    (a, _, pa, _), (b, _, pb, _) = _epoch(ds)
    want = golds["dataset"]["cases"]["square"]["batches"][0]["im"][1]
    assert a.shape[0] == 3 and b.shape[0] == 1 and all(torch.equal(x, want) for x in (*a, *b)) and pa == (dc.paths()[1],) * 3 and pb == (dc.paths()[1],)
    ds.set_indices(None)
    assert torch.equal(_epoch(ds)[0][0], dc.expected_images(golds["dataset"], "square", 0))


def test_two_epochs_with_prefetch_are_two_epochs_without(dev):
    c = ac.CASES["wild"]   # mixup and a repeating draw
    with_, without = (_train(ac.make_images(), ac.make_labels(), c, dev, p) for p in (1, 0))
    _seed(11)
    a = _epoch(with_) + _epoch(with_)
    end = random.random(), float(np.random.random())
    _seed(11)
    b = _epoch(without) + _epoch(without)
    assert len(a) == 8 and _same_epochs(a, b) and (random.random(), float(np.random.random())) == end
    assert not _same_epochs(a[:4], a[4:])   # (the second epoch drew on: the comparison is not of one epoch with itself)


@pytest.mark.parametrize("prefetch", [0, 1])
def test_get_batch_out_of_order_is_the_iterated_batch(prefetch, dev):
    c = ac.CASES["wild"]
    ds = _train(ac.make_images(), ac.make_labels(), c, dev, prefetch)
    _seed(5)
    items = [ds.draw_batch(k) for k in range(len(ds))]
    want = _epoch(ds, 5)
    for k in (3, 0, 2, 2, 1):
        im, targets, paths, shapes = ds.get_batch(k, items=items[k])
        assert _same_epochs([(im.cpu(), targets.cpu(), paths, shapes)], [want[k]]), f"batch {k} out of order"
    # and between the batches of a running epoch: what was staged ahead keeps its half
    _seed(5)
    got = []
    for k, batch in enumerate(ds):
        got.append(tuple(t.cpu() if isinstance(t, torch.Tensor) else t for t in batch))
        other = (k + 2) % len(ds)
        im, targets, paths, shapes = ds.get_batch(other, items=items[other])
        assert _same_epochs([(im.cpu(), targets.cpu(), paths, shapes)], [want[other]]), f"batch {other} while the epoch stands at {k}"
    assert _same_epochs(got, want)
    val = _val("rect_pad05", dev, store="host", prefetch=prefetch)
    whole = _epoch(val)
    for k in (2, 0, 1):
        im, targets, paths, shapes = val.get_batch(k)
        assert _same_epochs([(im.cpu(), targets.cpu(), paths, shapes)], [whole[k]])
    val._store.check()


# ---- the export alone, on a synthetic host arena -----------------------------------------------------------------------------------------------------------------------

def _sizes(chunk):
    """Image sizes are 3 h w bytes, so of chunk - 16, chunk and chunk + 16 at most one is an image size: each stands here as the largest multiple of 3 that has that
    slot (the image's bytes rounded up to 16) -- the slots, on which every chunk decision of the kernel rests, are exactly 16, chunk - 16, chunk, chunk + 16 and
    4 chunk + 48, and all but possibly one of the images end inside their slot's last 16 bytes."""
    sizes = [3] + [s // 3 * 3 for s in (chunk - 16, chunk, chunk + 16, 4 * chunk + 48)]
    assert [-(-s // 16) * 16 for s in sizes] == [16, chunk - 16, chunk, chunk + 16, 4 * chunk + 48]
    return sizes


class _Synthetic:
    """n images of the given byte sizes (h = bytes / 3, w = 1) in a pinned arena whose gap bytes are NOT zero, source records on the device, a ring pre-filled with a
    canary inside a larger buffer, a destination table pre-filled with a pattern"""

    def __init__(self, sizes, ring_bytes, dev, seed=0):
        from yolov3_amd import dataset, ops

        rng = np.random.default_rng(seed)
        self.sizes, self.n, self.dev = list(sizes), len(sizes), dev
        self.slots = np.array([-(-s // 16) * 16 for s in sizes], dtype=np.int64)
        self.offsets = np.concatenate([[0], np.cumsum(self.slots)])
        self.arena = torch.empty(int(self.offsets[-1]), dtype=torch.uint8, pin_memory=True)
        host = self.arena.numpy()
        host[:] = 0xEE
        self.images = []
        for i, s in enumerate(sizes):
            self.images.append(rng.integers(0, 256, s, dtype=np.uint8))
            host[self.offsets[i] : self.offsets[i] + s] = self.images[i]
        self.rec = np.zeros(self.n, dtype=dataset._RECORD)
        for i, s in enumerate(sizes):
            self.rec[i] = (self.offsets[i], s // 3, 1, i, i + 1, 64, 64)
        self.src = torch.from_numpy(self.rec.view(np.uint8).reshape(-1).copy()).to(dev)
        self.buffer = torch.full((ring_bytes + 4096,), CANARY, dtype=torch.uint8, device=dev)
        self.ring = self.buffer[:ring_bytes]
        self.dst = torch.full((32 * self.n,), 0x5A, dtype=torch.uint8, device=dev)
        self.status = torch.zeros(1, dtype=torch.int32, device=dev)
        self.chunk = ops.dataset_stage_chunk_bytes()

    def jobs(self, rows, chunks=None):
        """rows of (image, slot offset) -> the DEVICE job table with running chunk counts (`chunks`: per job, default its slot's)"""
        counts = [-(-int(self.slots[i]) // self.chunk) if 0 <= i < self.n else 1 for i, _ in rows] if chunks is None else chunks
        table = np.array([[i, at, run] for (i, at), run in zip(rows, np.cumsum(counts))], dtype=np.int64).reshape(-1, 3)
        return torch.from_numpy(table).to(self.dev), int(table[-1, 2]) if len(table) else 0

    def stage(self, rows, chunks=None, arena=None, src=None):
        from yolov3_amd import ops

        jobs, n_chunks = self.jobs(rows, chunks)
        ops.dataset_stage(self.arena if arena is None else arena, self.src if src is None else src, self.n, jobs, len(rows), n_chunks, self.ring, self.dst, self.status)
        torch.cuda.synchronize()

    def check(self, staged, skipped=0):
        """every slot of `staged` {image: slot offset} equals its image with a zero gap, every other byte of the buffer holds the canary, the records of `staged` are the
        source's with the slot's offset and every other record is untouched"""
        from yolov3_amd import dataset

        buf = self.buffer.cpu().numpy()
        want = np.full_like(buf, CANARY)
        for i, at in staged.items():
            want[at : at + self.sizes[i]] = self.images[i]
            want[at + self.sizes[i] : at + self.slots[i]] = 0
        bad = np.nonzero(buf != want)[0]
        assert len(bad) == 0, f"{len(bad)} bytes differ, first at {bad[:4].tolist()}"
        dst = self.dst.cpu().numpy()
        rec = dst.view(dataset._RECORD)
        for i in range(self.n):
            if i in staged:
                w = self.rec[i].copy()
                w["offset"] = staged[i]
                assert rec[i] == w, f"record {i}"
            else:
                assert (dst[32 * i : 32 * i + 32] == 0x5A).all(), f"record {i} was written"
        assert int(self.status.item()) == skipped


def test_the_export_copies_images_around_the_chunk_size(dev):
    from yolov3_amd import ops

    chunk = ops.dataset_stage_chunk_bytes()
    sizes = _sizes(chunk) + [48, 3 * 1000]   # two more images that no job names: their records stay untouched
    gap = 32                                  # canary bytes between the slots, and before the first
    order = [4, 0, 2, 1, 3]                   # not in the order of the arena
    staged, at = {}, gap
    for i in order:
        staged[i] = at
        at += -(-sizes[i] // 16) * 16 + gap
    s = _Synthetic(sizes, at, dev)
    assert [s.slots[i] for i in order] == [4 * chunk + 48, 16, chunk, chunk - 16, chunk + 16]
    s.stage([], None)                         # m = 0: nothing is launched, nothing is written
    s.check({})
    s.stage([(i, staged[i]) for i in order])
    s.check(staged)
    s.stage([(0, staged[1])])                 # a later batch moves image 0 into another slot of the same ring: the record follows
    assert torch.equal(s.buffer[staged[1] : staged[1] + 16].cpu(), torch.tensor(list(s.images[0]) + [0] * 13, dtype=torch.uint8))
    assert int(s.dst.cpu().numpy().view(s.rec.dtype)[0]["offset"]) == staged[1]


def test_jobs_that_do_not_fit_are_skipped_and_counted(dev):
    """the clamp itself: a skipped job's addresses are never formed, so nothing here can fault"""
    from yolov3_amd import dataset, ops

    chunk = ops.dataset_stage_chunk_bytes()
    s = _Synthetic([48, 3 * 40, 48, chunk + 48], 4096, dev)
    past = s.rec.copy()
    past[0]["offset"] = s.arena.numel() - 16          # image 0: 48 bytes from 16 bytes before the arena's end
    past[2]["h"] = (s.arena.numel() // 3) + 1         # image 2: larger than the whole arena
    src = torch.from_numpy(past.view(np.uint8).reshape(-1).copy()).to(dev)
    s.stage([(0, 0), (1, 4096 - 112), (2, 256)], src=src)   # the source range ends past host_bytes; the slot of 128 bytes ends past the ring; and again the source
    s.check({}, skipped=3)
    s.stage([(1, 512)], src=src)                      # the same image in a slot that fits, from the same table: copied
    s.check({1: 512}, skipped=3)
    s.stage([(7, 0), (-1, 0), (1, -16), (1, 8), (1, 1 << 40), (3, 0)], chunks=[1, 1, 1, 1, 1, 2])   # no such image; a negative, a misaligned and a far slot; a slot larger than the ring
    s.check({1: 512}, skipped=9)
    s.stage([(1, 1024)], chunks=[2])                  # a chunk count that is not the slot's
    s.check({1: 512}, skipped=10)
    assert dataset._RECORD.itemsize == 32


def test_a_pageable_arena_is_refused_and_nothing_is_launched(dev):
    from yolov3_amd import DeviceDataset, _lib

    s = _Synthetic([48, 96], 1024, dev)
    pageable = torch.from_numpy(s.arena.numpy().copy())
    assert not pageable.is_pinned() and s.arena.is_pinned()
    with pytest.raises(_lib.Y3Error, match="y3_dataset_stage: the host arena's 144 bytes are not pinned, mapped host memory"):
        s.stage([(0, 0), (1, 64)], arena=pageable)
    torch.cuda.synchronize()
    s.check({})
    with pytest.raises(_lib.Y3Error, match="not pinned, mapped host memory"):   # device memory is no host arena either
        s.stage([(0, 0)], arena=SimpleNamespace(is_cuda=False, dtype=torch.uint8, dim=lambda: 1, is_contiguous=lambda: True, data_ptr=s.buffer.data_ptr, numel=lambda: 144))
    s.check({})
    s.stage([(0, 0), (1, 64)])   # the runtime is not left in an error state: the pinned arena goes through
    s.check({0: 0, 1: 64})
    ds = DeviceDataset(dc.make_images(), dc.make_labels(), img_size=dc.IMG_SIZE, batch_size=dc.BATCH, rect=False, device=dev, store="host")
    assert ds._store.arena.is_pinned()   # the datasets never hand the export anything else
