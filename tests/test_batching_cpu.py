"""CPU tests of the device-side batch preparation (csrc/batch_edge.hip, yolov3_amd/batching.py): the public surface, the C ABI's argument validation without a
GPU, and the host halves -- the --multi-scale size draw and the --quad labels -- against the fixtures of the unmodified reference
(tests/golden/make_batching_golden.py)."""
import random
import re
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
NEW_SYMBOLS = ["y3_resize_bilinear", "y3_quad_collate_u8"]
F16, BF16, F32, U8 = 0, 1, 2, 3


@pytest.fixture(scope="module")
def lib():
    from yolov3_amd import _lib, build

    build.build(verbose=False)
    return _lib.lib()


@pytest.fixture(scope="module")
def gold(golden_dir):
    return torch.load(golden_dir / "batching.pt", weights_only=True)   # data only


def collated(labels):
    """the loader's collate_fn: per-image labels -> one (n, 6) tensor with the image index in column 0"""
    out = [lb.clone() for lb in labels]
    for i, lb in enumerate(out):
        lb[:, 0] = i
    return torch.cat(out, 0)


def test_public_names_import():
    import yolov3_amd
    from yolov3_amd import batching, multi_scale_size, ops, preprocess_batch, quad_collate, resize_batch

    assert batching.multi_scale_size is multi_scale_size and batching.resize_batch is resize_batch
    assert batching.preprocess_batch is preprocess_batch and batching.quad_collate is quad_collate is yolov3_amd.quad_collate
    assert callable(ops.resize_bilinear) and callable(ops.quad_collate_u8) and callable(batching.quad_labels)


def test_new_symbols_are_declared_bound_and_exported_at_abi_6(lib):
    from yolov3_amd import _lib

    header = (ROOT / "include" / "yolov3_hip.h").read_text()
    declared = set(re.findall(r"\b(y3_[a-z0-9_]+)\s*\(", header))
    assert set(NEW_SYMBOLS) <= declared and set(NEW_SYMBOLS) <= set(_lib.exported_symbols())
    assert "#define Y3_ABI_VERSION 6" in re.sub(r"[ \t]+", " ", header) and lib.y3_abi_version() == 6 == _lib.ABI_VERSION
    assert ("batch_edge.hip", ["-ffp-contract=off"]) in __import__("yolov3_amd.build", fromlist=["SOURCES"]).SOURCES
    assert all(s in (ROOT / "INTEGRATION.md").read_text() for s in NEW_SYMBOLS)
    # one definition of the bilinear arithmetic, included by both kernels
    for unit in ("val_edge.hip", "batch_edge.hip"):
        text = (ROOT / "yolov3_amd" / "csrc" / unit).read_text()
        assert '#include "y3_bilinear.h"' in text and "y3_bilinear_tap(" in text and "y3_bilinear_mix(" in text


def test_new_exports_reject_bad_arguments_without_a_gpu(lib):
    P = 1 << 20   # a fake, aligned device address: validation never dereferences it

    def fails(status, *needles):
        msg = lib.y3_last_error()
        assert status != 0 and all(n in msg for n in needles), (status, msg)

    rb = lib.y3_resize_bilinear
    fails(rb(None, U8, 2, 3, 64, 64, P, F32, 96, 96, 255.0, None), b"y3_resize_bilinear", b"null")
    fails(rb(P, U8, 2, 3, 64, 64, None, F32, 96, 96, 255.0, None), b"y3_resize_bilinear", b"null")
    for geo in ((-1, 3, 64, 64, 96, 96), (2, 0, 64, 64, 96, 96), (2, 3, 0, 64, 96, 96), (2, 3, 64, -4, 96, 96), (2, 3, 64, 64, 0, 96), (2, 3, 64, 64, 96, -1)):
        n, c, h, w, oh, ow = geo
        fails(rb(P, U8, n, c, h, w, P, F32, oh, ow, 255.0, None), b"y3_resize_bilinear", b"bad geometry")
    fails(rb(P, 7, 2, 3, 64, 64, P, F32, 96, 96, 255.0, None), b"y3_resize_bilinear", b"unsupported source dtype 7")
    fails(rb(P, U8, 2, 3, 64, 64, P, U8, 96, 96, 255.0, None), b"y3_resize_bilinear", b"unsupported output dtype 3")
    fails(rb(P, F16, 2, 3, 64, 64, P, -1, 96, 96, 1.0, None), b"y3_resize_bilinear", b"unsupported output dtype -1")
    fails(rb(P, U8, 2, 3, 64, 64, P, F32, 96, 96, 0.0, None), b"y3_resize_bilinear", b"divisor", b"positive")
    fails(rb(P, U8, 2, 3, 64, 64, P, F32, 96, 96, -255.0, None), b"y3_resize_bilinear", b"divisor", b"positive")
    fails(rb(P, U8, 2, 3, 64, 64, P, F32, 96, 96, float("nan"), None), b"y3_resize_bilinear", b"divisor")
    fails(rb(P, U8, 1 << 20, 1 << 12, 64, 64, P, F32, 96, 96, 255.0, None), b"y3_resize_bilinear", b"too many planes")
    fails(rb(P, U8, 1, 1, 1 << 16, 1 << 16, P, F32, 96, 96, 255.0, None), b"y3_resize_bilinear", b"too large")
    fails(rb(P, U8, 1, 1, 64, 64, P, F32, 1 << 16, 1 << 16, 255.0, None), b"y3_resize_bilinear", b"too large")
    assert rb(P, U8, 0, 3, 64, 64, P, F32, 96, 96, 255.0, None) == 0   # an empty batch launches nothing

    qc = lib.y3_quad_collate_u8
    fails(qc(None, 8, 3, 6, 10, P, P, None), b"y3_quad_collate_u8", b"null")
    fails(qc(P, 8, 3, 6, 10, None, P, None), b"y3_quad_collate_u8", b"null")
    fails(qc(P, 8, 3, 6, 10, P, None, None), b"y3_quad_collate_u8", b"null")
    for bs, c, h, w in ((-4, 3, 6, 10), (8, 0, 6, 10), (8, 3, 0, 10), (8, 3, 6, -1)):
        fails(qc(P, bs, c, h, w, P, P, None), b"y3_quad_collate_u8", b"bad geometry")
    fails(qc(P, 6, 3, 6, 10, P, P, None), b"y3_quad_collate_u8", b"batch size 6", b"multiple of 4")
    fails(qc(P, 1 << 20, 1 << 12, 6, 10, P, P, None), b"y3_quad_collate_u8", b"too many planes")
    fails(qc(P, 4, 1, 1 << 15, 1 << 15, P, P, None), b"y3_quad_collate_u8", b"too large")
    assert qc(P, 0, 3, 6, 10, P, P, None) == 0


def test_multi_scale_size_draws_what_the_reference_draws(gold):
    from yolov3_amd import multi_scale_size

    assert gold["draws"][(0, 640, (640, 640))]["sizes"][:3] == [[704, 704], [736, 736], [352, 352]]
    assert gold["draws"][(0, 640, (384, 640))]["sizes"][:3] == [[448, 704], [448, 736], [224, 352]]
    assert gold["draws"][(0, 416, (416, 416))]["sizes"][:4] == [[640, 640], [384, 384], [576, 576], None]
    assert len(gold["draws"]) == 16
    for (seed, imgsz, shape), g in gold["draws"].items():
        assert len(g["sizes"]) == 8
        random.seed(seed)   # the module's generator, as train.py uses it ...
        got = [multi_scale_size(torch.Size((16, 3, *shape))[2:], imgsz, gold["gs"]) for _ in g["sizes"]]
        assert [None if s is None else list(s) for s in got] == g["sizes"], (seed, imgsz, shape)
        assert random.random() == g["next_random"]
        rng = random.Random(seed)   # ... and a private one
        got = [multi_scale_size(shape, imgsz, gold["gs"], rng=rng) for _ in g["sizes"]]
        assert [None if s is None else list(s) for s in got] == g["sizes"] and rng.random() == g["next_random"]


def test_quad_labels_match_collate_fn4_bit_for_bit(gold):
    from yolov3_amd.batching import quad_labels

    labels = gold["quad_in"]["labels"]
    assert len(labels) == 8 and min(len(lb) for lb in labels) == 0 and max(len(lb) for lb in labels) == 5
    targets = collated(labels)
    before = targets.clone()
    seen = set()
    for seed, g in gold["quad"].items():
        got = quad_labels(targets, 8, g["flags"])
        assert got.dtype == g["labels"].dtype and torch.equal(got, g["labels"]), seed
        seen.update(enumerate(g["flags"]))
    assert seen == {(0, True), (0, False), (1, True), (1, False)}   # both branches in both groups
    assert torch.equal(targets, before)   # the caller's tensor is left alone
    assert quad_labels(torch.zeros(0, 6), 0, []).shape == (0, 6)


def test_quad_collate_draws_once_per_group_and_rejects_cpu_images(gold, monkeypatch):
    from yolov3_amd import batching, ops, preprocess_batch, quad_collate, resize_batch

    imgs, targets = gold["quad_in"]["imgs"], collated(gold["quad_in"]["labels"])
    with pytest.raises(RuntimeError, match="no CPU"):
        quad_collate(imgs, targets)
    with pytest.raises(RuntimeError, match="no CPU"):
        resize_batch(imgs, (12, 20))
    with pytest.raises(RuntimeError, match="no CPU"):
        ops.resize_bilinear(imgs.float(), (12, 20))
    with pytest.raises(RuntimeError, match="no CPU"):
        ops.quad_collate_u8(imgs, torch.zeros(2, dtype=torch.uint8))
    with pytest.raises(TypeError, match="uint8"):
        preprocess_batch(imgs.float(), 640)
    # with the launch stubbed out the host side runs here: the draws, their order and the labels are the reference's
    monkeypatch.setattr(ops, "require_gpu", lambda t, what: None)
    monkeypatch.setattr(ops, "quad_collate_u8", lambda x, flags: ("launched", flags.tolist()))
    for seed, g in gold["quad"].items():
        random.seed(seed)
        (tag, flags), lb4 = quad_collate(imgs, targets)
        assert tag == "launched" and flags == [int(f) for f in g["flags"]] and torch.equal(lb4, g["labels"])
        assert random.random() == g["next_random"]
        rng = random.Random(seed)
        assert torch.equal(batching.quad_collate(imgs, targets, rng=rng)[1], g["labels"]) and rng.random() == g["next_random"]
    with pytest.raises(ValueError, match="multiple of 4"):
        quad_collate(imgs[:6], targets)
    with pytest.raises(TypeError, match="uint8"):
        quad_collate(imgs.float(), targets)
    with pytest.raises(TypeError, match=r"\(n, 6\)"):
        quad_collate(imgs, targets[:, :5])
