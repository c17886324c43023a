"""CPU tests of the host-resident image store (yolov3_amd/dataset.py: plan_slots, ring_half_bytes, stage_jobs, check_store; csrc/dataset_stage.hip through its export's
argument check): the slot planner is a pure function of the drawn items, the half of the ring is sized for the worst batch, the keywords are refused before anything is
pinned or uploaded, and y3_dataset_stage refuses what it can be given without a device in the text of its family.  No GPU is needed: no call here launches."""
import re
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests"))

import augment_cases as ac  # noqa: E402

from yolov3_amd import _lib, augment  # noqa: E402
from yolov3_amd import dataset as ds  # noqa: E402

P = 1 << 20   # a fake, aligned device address: validation never dereferences it


def _slots():
    """the 16-byte aligned sizes of the twelve fixture images (a long side of 64: every size is a multiple of 16 already, all different)"""
    return np.array([-(-im.nbytes // 16) * 16 for im in ac.make_images()], dtype=np.int64)


def test_the_planner_stages_a_repeated_image_once():
    slots = _slots()
    tail = ac.CASES["wild"]["indices"][12:]
    assert tail == [5, 5, 2, 5]   # the epoch of `wild` ends in a batch that repeats an image
    unique, offsets = ds.plan_slots(tail, slots, ds.ring_half_bytes(slots, 1, 4))
    assert unique.tolist() == [5, 2] and offsets.tolist() == [0, int(slots[5])] and unique.dtype == offsets.dtype == np.int64
    # the images of a mosaic batch as the train-mode sets collect them: every tile of every mosaic, in draw order
    needs = [3, 7, 3, 1, 7, 7, 0, 11, 3, 3, 3, 3]
    unique, offsets = ds.plan_slots(needs, slots, ds.ring_half_bytes(slots, 4, 4))
    assert unique.tolist() == [3, 7, 1, 0, 11]   # once each, in the order of the first draw
    assert ds.plan_slots(needs, slots, 1 << 30)[1].tolist() == offsets.tolist() and ds.plan_slots(list(reversed(needs)), slots, 1 << 30)[0].tolist() == [3, 11, 0, 7, 1]   # pure
    empty = ds.plan_slots([], slots, 16)
    assert len(empty[0]) == len(empty[1]) == 0


def test_slots_are_aligned_and_disjoint():
    slots = _slots()
    rng = np.random.default_rng(0)
    half = ds.ring_half_bytes(slots, 8, 4)
    for _ in range(50):
        needs = rng.integers(0, 12, size=rng.integers(1, 33)).tolist()
        unique, offsets = ds.plan_slots(needs, slots, half)
        assert sorted(unique.tolist()) == sorted(set(needs)) and len(set(unique.tolist())) == len(unique)
        assert (offsets % 16 == 0).all() and offsets[0] == 0
        ends = offsets + slots[unique]
        assert (offsets[1:] >= ends[:-1]).all() and ends[-1] <= half   # back to back: no two slots share a byte, and the last ends inside the half
        jobs = ds.stage_jobs(unique, offsets, slots, 4096)
        assert jobs.dtype == np.int64 and jobs.shape == (len(unique), 3) and jobs[:, 0].tolist() == unique.tolist() and jobs[:, 1].tolist() == offsets.tolist()
        assert np.diff(np.concatenate([[0], jobs[:, 2]])).tolist() == [-(-int(s) // 4096) for s in slots[unique]]   # running chunk counts


def test_the_half_holds_the_worst_batch():
    slots = _slots()
    desc = np.sort(slots)[::-1]
    assert ds.ring_half_bytes(slots, 1, 4) == int(desc[:4].sum())    # DeviceDataset, a rect train set, mosaic=False: one image per item
    assert ds.ring_half_bytes(slots, 4, 2) == int(desc[:8].sum())    # a mosaic: four
    assert ds.ring_half_bytes(slots, 8, 1) == int(desc[:8].sum())    # mixup: eight
    assert ds.ring_half_bytes(slots, 4, 4) == ds.ring_half_bytes(slots, 8, 4) == int(slots.sum())   # min(n, t * batch_size): never more than the set
    assert ds.ring_half_bytes(slots, 1, 1) == int(slots.max())


def test_a_batch_that_exceeds_the_half_raises():
    slots = _slots()
    half = ds.ring_half_bytes(slots, 1, 2)
    big = np.argsort(slots)[::-1][:3].tolist()   # a hand-made item list: the three largest images into a half sized for two
    with pytest.raises(ValueError, match="ring half holds"):
        ds.plan_slots(big, slots, half)
    ds.plan_slots(big[:2], slots, half)
    ds.plan_slots(big[:2] + big[:2], slots, half)   # (repeats take no room)
    with pytest.raises(ValueError, match=r"outside \[0, 12\)"):
        ds.plan_slots([0, 12], slots, half)
    with pytest.raises(ValueError, match=r"outside \[0, 12\)"):
        ds.plan_slots([-1], slots, half)


HYP = dict(ac.CASES["low"]["hyp"])


def _dataset(**kw):
    from yolov3_amd import DeviceDataset

    return DeviceDataset(ac.make_images(), ac.make_labels(), img_size=64, batch_size=4, rect=False, **kw)


def _train(**kw):
    from yolov3_amd import DeviceTrainDataset

    return DeviceTrainDataset(ac.make_images(), ac.make_labels(), HYP, img_size=ac.IMG_SIZE, batch_size=ac.BATCH, stride=ac.STRIDE, **kw)


def _rect(**kw):
    from yolov3_amd import DeviceRectTrainDataset

    return DeviceRectTrainDataset(ac.make_images(), ac.make_labels(), HYP, img_size=64, batch_size=4, stride=16, **kw)


@pytest.mark.parametrize("build", [_dataset, _train, _rect])
def test_the_keywords_are_refused_before_anything_is_pinned_or_uploaded(build, monkeypatch):
    def never(*a, **k):
        raise AssertionError("something was pinned or uploaded before the refusal")

    monkeypatch.setattr(ds, "_upload_arena", never)
    monkeypatch.setattr(ds, "_upload", never)
    monkeypatch.setattr(ds, "HostStore", never)
    monkeypatch.setattr(ds, "_device", never)
    for store in ("hbm", "pinned", None, 0):
        with pytest.raises(ValueError, match="store = "):
            build(store=store)
    for prefetch in (2, -1, 0.5, "1", True):
        with pytest.raises(ValueError, match="prefetch = "):
            build(store="host", prefetch=prefetch)
    with pytest.raises(ValueError, match="prefetch = 1 with store = 'device'"):
        build(prefetch=1)
    with pytest.raises(ValueError, match="prefetch = 1 with store = 'device'"):
        build(store="device", prefetch=1)
    assert ds.check_store("x", "host", None) == 1 and ds.check_store("x", "host", 0) == 0 and ds.check_store("x", "device", None) == 0 and ds.check_store("x", "device", 0) == 0


def test_from_dataset_hands_the_keywords_on():
    from types import SimpleNamespace

    from yolov3_amd import DeviceDataset, DeviceRectTrainDataset, DeviceTrainDataset

    ref = SimpleNamespace(ims=ac.make_images(), im_hw0=ac.hw0(), im_hw=ac.hw(), labels=ac.make_labels(), segments=[[] for _ in range(12)], im_files=ac.paths(), rect=False,
                          img_size=ac.IMG_SIZE, stride=ac.STRIDE, augment=True, mosaic=True, hyp=HYP, indices=range(12))
    with pytest.raises(ValueError, match="store = 'disk'"):
        DeviceTrainDataset.from_dataset(ref, batch_size=4, store="disk")
    with pytest.raises(ValueError, match="prefetch = 1 with store = 'device'"):
        DeviceTrainDataset.from_dataset(ref, batch_size=4, prefetch=1)
    ref.rect = True
    with pytest.raises(ValueError, match="prefetch = 3"):
        DeviceRectTrainDataset.from_dataset(ref, batch_size=4, store="host", prefetch=3)
    ref.augment, ref.rect = False, False
    with pytest.raises(ValueError, match="store = 'disk'"):
        DeviceDataset.from_dataset(ref, batch_size=4, store="disk")


def test_the_items_of_a_batch_name_at_most_four_images_or_eight_with_mixup():
    import random

    state = random.getstate(), np.random.get_state()
    try:
        random.seed(1)
        np.random.seed(1)
        hyp = dict(ac.CASES["wild"]["hyp"], mixup=1.0)
        items = [augment.draw_item(i, ac.hw(), hyp, ac.IMG_SIZE) for i in range(4)]
        needs = augment._DeviceAugmentDataset._needs(items)
        assert len(needs) == 32 and all(len(it.mosaics) == 2 for it in items) and set(needs) <= set(range(12))
        letter = [augment.draw_item(i, ac.hw(), hyp, ac.IMG_SIZE, mosaic=False) for i in range(4)]
        assert augment._DeviceAugmentDataset._needs(letter) == [0, 1, 2, 3]
    finally:
        random.setstate(state[0])
        np.random.set_state(state[1])


def test_the_header_declares_the_exports_and_the_abi_stays_6():
    header = re.sub(r"\s+", " ", (ROOT / "include" / "yolov3_hip.h").read_text())
    assert len(re.findall(r"\bint y3_dataset_stage\(", header)) == 1 and len(re.findall(r"\bint64_t y3_dataset_stage_chunk_bytes\(void\);", header)) == 1   # declared once
    import ctypes as C

    V, I32, I64 = C.c_void_p, C.c_int32, C.c_int64
    assert _lib._SIGNATURES["y3_dataset_stage"] == (C.c_int, [V, I64, V, I64, V, I32, I64, V, I64, V, V, V])
    assert _lib._SIGNATURES["y3_dataset_stage_chunk_bytes"] == (I64, [])
    assert "y3_dataset_stage_chunk_bytes" in _lib._QUERIES and "y3_dataset_stage" not in _lib._QUERIES
    assert _lib.ABI_VERSION == 6 and "#define Y3_ABI_VERSION 6" in (ROOT / "include" / "yolov3_hip.h").read_text()
    assert ("dataset_stage.hip", ["-ffp-contract=off"]) in __import__("yolov3_amd.build", fromlist=["SOURCES"]).SOURCES


@pytest.fixture(scope="module")
def lib():
    from yolov3_amd import build

    build.build(verbose=False)
    return _lib.lib()


# y3_dataset_stage(host_arena, host_bytes, src_images, n_images, jobs, m, n_chunks, ring, ring_bytes, dst_images, status, stream)
VALID = dict(host_arena=P, host_bytes=4096, src_images=P, n_images=12, jobs=P, m=2, n_chunks=2, ring=P, ring_bytes=4096, dst_images=P, status=P, stream=None)
GEOMETRY = "y3_dataset_stage: bad geometry ({n_images} images in 1 .. 2^31 - 1, {m} jobs in 0 .. 8192, {n_chunks} chunks, a host arena of {host_bytes} and a ring of {ring_bytes} bytes, " \
           "both positive multiples of 16)"
FAULTS = [
    ("host_arena", None, "y3_dataset_stage: null argument"), ("src_images", None, "y3_dataset_stage: null argument"), ("jobs", None, "y3_dataset_stage: null argument"),
    ("ring", None, "y3_dataset_stage: null argument"), ("dst_images", None, "y3_dataset_stage: null argument"), ("status", None, "y3_dataset_stage: null argument"),
    ("m", -1, GEOMETRY), ("m", 8193, GEOMETRY), ("n_images", 0, GEOMETRY), ("n_chunks", -1, GEOMETRY), ("n_chunks", 1 << 31, GEOMETRY), ("host_bytes", 0, GEOMETRY),
    ("host_bytes", 4104, GEOMETRY), ("ring_bytes", 4100, GEOMETRY), ("ring_bytes", -16, GEOMETRY),
    ("ring", P + 8, "y3_dataset_stage: the host arena and the ring must be 16-byte aligned"), ("host_arena", P + 4, "y3_dataset_stage: the host arena and the ring must be 16-byte aligned"),
    ("src_images", P + 4, "y3_dataset_stage: the record tables and the jobs must be 8-byte, the status word 4-byte aligned"),
    ("dst_images", P + 4, "y3_dataset_stage: the record tables and the jobs must be 8-byte, the status word 4-byte aligned"),
    ("jobs", P + 4, "y3_dataset_stage: the record tables and the jobs must be 8-byte, the status word 4-byte aligned"),
    ("status", P + 2, "y3_dataset_stage: the record tables and the jobs must be 8-byte, the status word 4-byte aligned"),
]


@pytest.mark.parametrize("arg,value,text", FAULTS, ids=[f"{a}={'P+' + str(v - P) if isinstance(v, int) and v > P else v}" for a, v, _ in FAULTS])
def test_the_export_refuses_one_bad_argument(lib, arg, value, text):
    header = re.sub(r"\s+", " ", (ROOT / "include" / "yolov3_hip.h").read_text())
    (params,) = re.findall(r"\bint y3_dataset_stage\(([^)]*)\);", header)
    names = [p.split()[-1].lstrip("*") for p in params.split(",")]
    assert names == list(VALID)
    args = dict(VALID, **{arg: value})   # exactly one argument differs from the valid set: the refusal comes before any call into the runtime
    status = lib.y3_dataset_stage(*args.values())
    assert status != 0 and lib.y3_last_error().decode() == text.format(**args)


def test_no_job_launches_nothing_and_the_chunk_is_a_multiple_of_16(lib):
    assert lib.y3_dataset_stage(*dict(VALID, m=0, n_chunks=0, jobs=None).values()) == 0   # fake addresses: a launch or a pointer query on them would fail
    chunk = lib.y3_dataset_stage_chunk_bytes()
    assert chunk >= 4096 and chunk % 16 == 0
