"""CPU tests of the device-side apply_classifier (yolov3_amd/crops.py, csrc/crops.hip): the fixture tests/golden/classifier_crops.pt, which the unmodified reference
wrote, against the NumPy statement of tests/classifier_crops_cases.py; the restated save_one_box on hand-worked boxes; the C ABI of the three exports; and every
refusal the host can make without a GPU, ahead of any launch."""
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

import classifier_crops_cases as cc

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "yolov3_hip.h"
EXPORTS = ["y3_classifier_boxes", "y3_crop_resize", "y3_keep_matching"]
P = 1 << 20   # a fake, aligned device address: validation never dereferences it


@pytest.fixture(scope="module")
def gold(golden_dir):
    return torch.load(golden_dir / "classifier_crops.pt", weights_only=True)


@pytest.fixture(scope="module")
def case():
    ims, x = cc.build_case()
    return ims, x, cc.statement(ims, x)


def test_fixture_against_the_statement(gold, case):
    ims, x, st = case
    assert tuple(gold["img1"]) == cc.IMG1 and gold["size"] == cc.SIZE and len(gold["x"]) == len(x) == 5
    assert [tuple(t.shape[:2]) for t in gold["images"]] == cc.SHAPES
    for t, im in zip(gold["images"], ims):
        assert t.dtype == torch.uint8 and np.array_equal(t.numpy(), im)
    n_full = 0
    for i, d in enumerate(x):
        if d is None or not len(d):
            assert all(gold[k][i] is None for k in ("boxes", "pred", "kept", "sha")) and (gold["x"][i] is None if d is None else gold["x"][i].shape == (0, 6))
            continue
        assert torch.equal(gold["x"][i], d) and 6 <= len(d) <= 10
        assert torch.equal(gold["boxes"][i], st["boxes"][i]) and gold["boxes"][i].dtype == torch.float32
        cuts = cc.cutouts(ims[i], gold["boxes"][i])
        assert all(c.shape[0] >= 1 and c.shape[1] >= 1 for c in cuts)
        assert gold["sha"][i] == [cc.sha(c) for c in st["crops"][i]]
        assert torch.equal(gold["pred"][i], st["pred"][i]) and torch.equal(gold["kept"][i], st["kept"][i])
        assert torch.equal(gold["kept"][i], d[d[:, 5].long() == gold["pred"][i]])
        for j in range(len(d)):
            if f"{i},{j}" in gold["full"]:
                assert np.array_equal(gold["full"][f"{i},{j}"].numpy(), st["crops"][i][j])
                n_full += 1
    assert n_full == len(gold["full"]) == len(cc.FULL_CROPS) <= 4
    cc.check_situations(ims, x, st)
    assert (ROOT / "tests" / "golden" / "classifier_crops.pt").stat().st_size < 1_000_000


def test_statement_pieces_on_hand_worked_values():
    # one detection, worked by hand: xyxy (100, 120, 140, 180) -> xywh (120, 150, 40, 60) -> square 60 -> 60 * 1.3 + 30 = 108 -> (66, 96, 174, 204)
    d = torch.tensor([[100.0, 120.0, 140.0, 180.0, 0.9, 1.0]])
    assert cc.classifier_boxes(d).tolist() == [[66.0, 96.0, 174.0, 204.0]]
    assert cc.classifier_boxes(d, 1.02, 10, False).tolist() == [[94.0, 114.0, 145.0, 185.0]]   # 40 * 1.02 + 10 = 50.8, 60 * 1.02 + 10 = 71.2
    # truncation, not rounding, and towards zero below it: centre 10, side 30 + 1.3 * 4 = 35.2 -> -7.6 -> -7, 27.6 -> 27
    assert cc.classifier_boxes(torch.tensor([[8.0, 8.0, 12.0, 12.0, 0.5, 0.0]])).tolist() == [[-7.0, -7.0, 27.0, 27.0]]
    # a 320 x 320 letterbox of a 160 x 320 image: gain 1, pad (0, 80); the clip cuts the square at the image's edge
    b = cc.scaled_boxes(d, (160, 320, 3))
    assert b.tolist() == [[66.0, 16.0, 174.0, 124.0]]
    im = np.arange(160 * 320 * 3, dtype=np.uint32).reshape(160, 320, 3).astype(np.uint8)
    (cut,) = cc.cutouts(im, b)
    assert cut.shape == (108, 108, 3) and np.array_equal(cut, im[16:124, 66:174])
    same = cc.crops_u8(im, b, 108)   # a resize to the cutout's own size is the identity
    assert np.array_equal(same[0], cut)
    f = cc.to_float(same)
    assert f.shape == (1, 3, 108, 108) and f.dtype == torch.float32 and float(f[0, 0, 5, 7]) == np.float32(cut[5, 7, 2]) / np.float32(255)


def test_save_one_box_on_hand_worked_boxes():
    im = np.random.RandomState(3).randint(0, 256, (100, 200, 3), dtype=np.uint8)
    crop, box = cc.save_one_box([50.0, 20.0, 90.0, 60.0], im)   # xywh (70, 40, 40, 40) -> 40 * 1.02 + 10 = 50.8 -> 44.6 .. 95.4, 14.6 .. 65.4
    assert box == [44, 14, 95, 65] and crop.shape == (51, 51, 3) and np.array_equal(crop, im[14:65, 44:95, ::-1])
    crop, box = cc.save_one_box([180.0, 80.0, 210.0, 110.0], im)   # xywh (195, 95, 30, 30) -> 40.6 -> 174.7 .. 215.3, 74.7 .. 115.3, clipped to 200 x 100
    assert box == [174, 74, 200, 100] and crop.shape == (26, 26, 3)
    crop, box = cc.save_one_box([2.0, 3.0, 12.0, 9.0], im, BGR=True)   # xywh (7, 6, 10, 6) -> 20.2, 16.12 -> -3.1 .. 17.1, -2.06 .. 14.06: towards zero, then the clip
    assert box == [0, 0, 17, 14] and np.array_equal(crop, im[0:14, 0:17])
    crop, box = cc.save_one_box([50.0, 20.0, 90.0, 40.0], im, gain=1.3, pad=30, square=True)   # the classifier's square: 40 * 1.3 + 30 = 82 -> 29 .. 111, -11 .. 71
    assert box == [29, 0, 111, 71]


def test_header_declares_the_exports_and_no_new_struct():
    from yolov3_amd import _lib, build

    for name in EXPORTS:
        assert name in _lib._SIGNATURES and name not in _lib._QUERIES
    V, I32, I64, F = (_lib.C.c_void_p, _lib.C.c_int32, _lib.C.c_int64, _lib.C.c_float)
    assert _lib._SIGNATURES["y3_classifier_boxes"] == (_lib.C.c_int, [V, I64, I32, V, I32, I32, F, F, I32, V, V])
    assert _lib._SIGNATURES["y3_crop_resize"] == (_lib.C.c_int, [V, I64, V, I64, V, V, V, I32, I32, V, I32, I64, I32, V, V])
    assert _lib._SIGNATURES["y3_keep_matching"] == (_lib.C.c_int, [V, I64, I32, V, V, I32, I32, V, I64, V, V, I64, I64, V, V, V])
    assert _lib.ABI_VERSION == 6 and len(_lib._H.structs) == 10 and len(re.findall(r"typedef\s+struct", HEADER.read_text())) == 10
    lib = build.build(verbose=False)
    listed = subprocess.run(["nm", "-D", "--defined-only", str(lib)], check=True, capture_output=True, text=True).stdout
    for name in EXPORTS:
        assert re.search(rf"\bT {name}$", listed, flags=re.M), name
    assert _lib.lib().y3_abi_version() == 6


@pytest.fixture(scope="module")
def lib():
    from yolov3_amd import _lib, build

    build.build(verbose=False)
    return _lib.lib()


def _parameters(name):
    header = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", " ", HEADER.read_text(), flags=re.S))
    (args,) = re.findall(rf"\bint {name}\(([^)]*)\);", header)
    return [a.split()[-1].lstrip("*") for a in args.split(",")]


VALID = {"arena_bytes": 4096, "n_images": 3, "bs": 3, "max_rows": 10, "dst_dtype": 2, "n_tiles": 5, "S": 224, "img_stride": 60, "row_stride": 6, "gain": 1.3, "pad": 30.0,
         "square": 1, "stream": None}
# (export, the one argument changed, its value, what the refusal says) -- in the order the exports test: null, geometry, alignment, dtype
REFUSALS = [
    ("y3_classifier_boxes", "rows", None, b"null argument"), ("y3_classifier_boxes", "boxes", None, b"null argument"),
    ("y3_classifier_boxes", "row_stride", 3, b"bad geometry (bs 3, rows 10, row stride 3)"), ("y3_classifier_boxes", "bs", -1, b"bad geometry"),
    ("y3_crop_resize", "arena", None, b"null argument"), ("y3_crop_resize", "status", None, b"null argument"), ("y3_crop_resize", "dst", None, b"null argument"),
    ("y3_crop_resize", "boxes", None, b"null argument"), ("y3_crop_resize", "prefix", None, b"null argument"),
    ("y3_crop_resize", "n_images", 2, b"bad geometry"), ("y3_crop_resize", "n_tiles", 31, b"bad geometry"), ("y3_crop_resize", "n_tiles", -1, b"bad geometry"),
    ("y3_crop_resize", "arena_bytes", 4098, b"bad geometry"), ("y3_crop_resize", "max_rows", 0, b"bad geometry"),
    ("y3_crop_resize", "S", 0, b"bad geometry (crops of 0 x 0, 1 .. 1024)"), ("y3_crop_resize", "S", 1025, b"bad geometry (crops of 1025 x 1025, 1 .. 1024)"),
    ("y3_crop_resize", "images", P + 4, b"8-byte"), ("y3_crop_resize", "prefix", P + 4, b"8-byte"), ("y3_crop_resize", "arena", P + 8, b"16-byte"),
    ("y3_crop_resize", "dst_dtype", 3, b"unsupported output dtype 3 (float16 / bfloat16 / float32)"), ("y3_crop_resize", "dst", P + 1, b"aligned to its element size"),
    ("y3_keep_matching", "rows", None, b"null argument"), ("y3_keep_matching", "out_counts", None, b"null argument"), ("y3_keep_matching", "classes", None, b"null argument"),
    ("y3_keep_matching", "bs", 4, b"bad geometry"), ("y3_keep_matching", "row_stride", 5, b"bad geometry (row stride 5)"), ("y3_keep_matching", "classes", P + 4, b"8-byte"),
]


@pytest.mark.parametrize("name,arg,value,says", REFUSALS, ids=[f"{r[0]}-{r[1]}={'P+' + str(r[2] - P) if isinstance(r[2], int) and r[2] > P else r[2]}" for r in REFUSALS])
def test_an_export_refuses_one_bad_argument(lib, name, arg, value, says):
    params = _parameters(name)
    assert arg in params
    args = [value if p == arg else VALID.get(p, P) for p in params]   # exactly one argument differs from a valid set: no call here launches
    status = getattr(lib, name)(*args)
    msg = lib.y3_last_error()
    assert status != 0 and msg.startswith(name.encode() + b":") and says in msg, (status, msg)


def test_refusals_come_in_the_order_of_the_augment_exports(lib):
    params = _parameters("y3_crop_resize")

    def call(**changed):
        status = lib.y3_crop_resize(*[changed.get(p, VALID.get(p, P)) for p in params])
        return status, lib.y3_last_error()

    assert b"null argument" in call(arena=None, S=0, dst_dtype=7)[1]
    assert b"bad geometry" in call(S=0, images=P + 4, dst_dtype=7)[1]
    assert b"aligned" in call(images=P + 4, dst_dtype=7)[1]
    assert b"dtype" in call(dst_dtype=7)[1]
    assert call(n_tiles=0) == (0, call(n_tiles=0)[1])   # no crop: nothing is launched, and nothing is refused


def _valid_cpu():
    rows = torch.zeros(2, 5, 6)
    return dict(rows=rows, counts_t=torch.tensor([2, 1], dtype=torch.int32), counts=[2, 1], img1_shape=(320, 320), images=[np.zeros((40, 50, 3), np.uint8)] * 2)


@pytest.mark.parametrize("change,error,says", [
    ({}, RuntimeError, "no CPU"),                                                              # a CPU tensor, everything else right
    ({"rows": torch.zeros(2, 5, 6, dtype=torch.float64)}, TypeError, "fp32"),
    ({"rows": torch.zeros(2, 5, 5)}, TypeError, "(bs, max_det, 6)"),
    ({"rows": torch.zeros(10, 6)}, TypeError, "(bs, max_det, 6)"),
    ({"counts_t": torch.tensor([2, 1])}, TypeError, "int32"),
    ({"counts_t": torch.tensor([2, 1, 0], dtype=torch.int32)}, TypeError, "(2,)"),
    ({"counts": [2, 6]}, ValueError, "host counts"),
    ({"counts": [2]}, ValueError, "host counts"),
    ({"size": 0}, ValueError, "1 .. 1024"),
    ({"size": 1025}, ValueError, "1 .. 1024"),
    ({"size": 224.0}, ValueError, "1 .. 1024"),
    ({"dtype": torch.uint8}, TypeError, "float16 / bfloat16 / float32"),
    ({"images": [np.zeros((40, 50, 3), np.uint8)]}, ValueError, "1 images for the detections of 2"),
    ({"images": [np.zeros((40, 50, 3), np.uint8)] * 3}, ValueError, "3 images for the detections of 2"),
    ({"images": [np.zeros((40, 50, 3), np.uint8), np.zeros((40, 50), np.uint8)]}, TypeError, "image 1"),
    ({"images": [np.zeros((40, 50, 3), np.uint8), np.zeros((40, 50, 3), np.float32)]}, TypeError, "image 1"),
    ({"img1_shape": (320,)}, ValueError, "img1_shape"),
])
def test_host_refusals_come_before_any_launch(monkeypatch, change, error, says):
    from yolov3_amd import crops, ops

    def launched(*a, **k):
        raise AssertionError("a launch or an upload before the refusal")

    for fn in ("classifier_boxes", "crop_resize", "keep_matching", "scale_boxes_raw"):
        monkeypatch.setattr(ops, fn, launched)
    monkeypatch.setattr(crops, "_upload", launched)
    monkeypatch.setattr(crops, "_upload_arena", launched)
    args = {**_valid_cpu(), **change}
    with pytest.raises(error, match=re.escape(says)):
        crops.classifier_crops(**args)
    with pytest.raises(error, match=re.escape(says)):
        crops.apply_classifier_batched(args.pop("rows"), args.pop("counts_t"), args.pop("counts"), cc.ToyClassifier(), **args)


def test_the_list_form_and_the_wrappers_refuse_cpu_tensors():
    import yolov3_amd
    from yolov3_amd import crops, ops

    assert yolov3_amd.apply_classifier is crops.apply_classifier and yolov3_amd.DeviceImages is crops.DeviceImages
    assert yolov3_amd.classifier_crops is crops.classifier_crops and yolov3_amd.apply_classifier_batched is crops.apply_classifier_batched
    model, im = cc.ToyClassifier(), np.zeros((40, 50, 3), np.uint8)
    with pytest.raises(RuntimeError, match="no CPU"):
        crops.apply_classifier([torch.zeros(2, 6)], model, (320, 320), [im])
    with pytest.raises(TypeError, match=re.escape("(n, 6) fp32")):
        crops.apply_classifier([torch.zeros(2, 5)], model, (320, 320), [im])
    assert crops.apply_classifier([None, torch.zeros(0, 6)], model, torch.zeros(1, 3, 320, 320), [im, im])[0] is None and not model.seen   # nothing to do: nothing is touched
    with pytest.raises(TypeError, match="image 0"):
        crops.DeviceImages([np.zeros((4, 5), np.uint8)])
    with pytest.raises(ValueError, match="no image"):
        crops.DeviceImages([])
    rows, counts = torch.zeros(2, 5, 6), torch.zeros(2, dtype=torch.int32)
    for call in (lambda: ops.classifier_boxes(rows, counts), lambda: ops.keep_matching(rows, counts, counts.long(), counts.long(), rows[..., :4], rows, rows),
                 lambda: ops.crop_resize(rows, rows, torch.zeros(2, 5, 4), counts, counts.long(), 0)):
        with pytest.raises(RuntimeError, match="no CPU"):
            call()
    assert hasattr(yolov3_amd.Detections, "crop")
