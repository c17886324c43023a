"""CPU tests of the output writers (yolov3_amd.outputs, y3_export_rows of csrc/val_edge.hip, the text half of yolov3_amd.Detections, the save_* arguments of
yolov3_amd.val.run_batches): the public surface, the C ABI's argument validation without a GPU, and the host formatting against the fixtures of the unmodified
reference (tests/golden/make_val_outputs_golden.py)."""
import inspect
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests"))

import val_outputs_cases as oc  # noqa: E402


@pytest.fixture(scope="module")
def lib():
    from yolov3_amd import _lib, build

    build.build(verbose=False)
    return _lib.lib()


@pytest.fixture(scope="module")
def gold(golden_dir):
    return torch.load(golden_dir / "val_outputs.pt", weights_only=False)


def test_fixture_matches_the_seeded_inputs(gold):
    for name in oc.CASES:
        c = oc.case(name)
        assert gold["cases"][name]["in_sum"] == oc.checksum(c) and gold["cases"][name]["counts"] == c["counts"], name


def test_public_names_import():
    import yolov3_amd
    from yolov3_amd import outputs

    for name in ("output_to_target", "save_one_txt", "save_one_json", "coco80_to_coco91_class", "save_txt_batched", "save_json_batched"):
        assert getattr(yolov3_amd, name) is getattr(outputs, name), name
    assert list(inspect.signature(outputs.output_to_target).parameters) == ["output", "max_det"] and inspect.signature(outputs.output_to_target).parameters["max_det"].default == 300
    assert list(inspect.signature(outputs.save_one_txt).parameters) == ["predn", "save_conf", "shape", "file"]
    assert list(inspect.signature(outputs.save_one_json).parameters) == ["predn", "jdict", "path", "class_map"]
    assert list(inspect.signature(outputs.save_txt_batched).parameters) == ["rows", "counts", "shapes0", "paths", "labels_dir", "save_conf", "detect"]
    assert list(inspect.signature(outputs.save_json_batched).parameters) == ["rows", "counts", "paths", "jdict", "class_map"]
    p = inspect.signature(yolov3_amd.run_batches).parameters
    assert [(k, p[k].default) for k in ("save_txt", "save_conf", "save_json", "save_dir", "class_map", "jdict")] == [
        ("save_txt", False), ("save_conf", False), ("save_json", False), ("save_dir", None), ("class_map", None), ("jdict", None)]


def test_package_import_does_not_import_pandas():
    code = "import sys, yolov3_amd; from yolov3_amd import Detections; assert 'pandas' not in sys.modules, 'pandas imported with the package'"
    subprocess.run([sys.executable, "-c", code], check=True, cwd=ROOT)


def test_export_symbol_is_declared_bound_and_exported_at_abi_6(lib):
    from yolov3_amd import _lib

    header = (ROOT / "include" / "yolov3_hip.h").read_text()
    assert re.search(r"\bint y3_export_rows\s*\(", header)
    assert "y3_export_rows" in _lib.exported_symbols() and len(_lib._SIGNATURES["y3_export_rows"][1]) == 18
    assert "#define Y3_ABI_VERSION 6" in re.sub(r"[ \t]+", " ", header) and lib.y3_abi_version() == 6 == _lib.ABI_VERSION
    assert (_lib.Y3_EXPORT_TARGET, _lib.Y3_EXPORT_TXT, _lib.Y3_EXPORT_JSON) == (0, 1, 2)
    assert re.search(r"Y3_EXPORT_TARGET = 0, Y3_EXPORT_TXT = 1, Y3_EXPORT_JSON = 2", header)
    nm = subprocess.run(["nm", "-D", "--defined-only", str(_lib.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    assert re.search(r" T y3_export_rows\b", nm)
    assert ("val_edge.hip", ["-ffp-contract=off"]) in __import__("yolov3_amd.build", fromlist=["SOURCES"]).SOURCES
    ops_src = (ROOT / "yolov3_amd" / "ops.py").read_text()
    callers = [f.name for f in (ROOT / "yolov3_amd").glob("*.py") if "y3_export_rows(" in f.read_text()]
    assert callers == ["ops.py"] and ops_src.count("y3_export_rows(") == 1   # every launch goes through ops.py


def test_export_rejects_bad_arguments_without_a_gpu(lib):
    P = 1 << 20   # a fake, aligned device address: validation never dereferences it

    def fails(status, *needles):
        msg = lib.y3_last_error()
        assert status == -1 and all(n in msg for n in (b"y3_export_rows", *needles)), (status, msg)

    #                   rows stride rs counts bs rows form limit round rev img0 sizes out cap offsets hist nc stream
    fails(lib.y3_export_rows(None, 1800, 6, P, 2, 300, 0, 0, 0, 0, 0, None, P, 600, P, None, 0, None), b"null")
    fails(lib.y3_export_rows(P, 1800, 6, P, 2, 300, 0, 0, 0, 0, 0, None, P, 600, None, None, 0, None), b"null")
    fails(lib.y3_export_rows(P, 1800, 6, P, 2, 300, 0, 0, 0, 0, 0, None, None, 600, P, None, 0, None), b"null")
    fails(lib.y3_export_rows(P, 1800, 6, P, 0, 300, 0, 0, 0, 0, 0, None, P, 600, P, None, 0, None), b"geometry", b"bs 0")
    fails(lib.y3_export_rows(P, 1800, 6, P, -3, 300, 0, 0, 0, 0, 0, None, P, 600, P, None, 0, None), b"geometry", b"bs -3")
    fails(lib.y3_export_rows(P, 1800, 5, P, 2, 300, 0, 0, 0, 0, 0, None, P, 600, P, None, 0, None), b"geometry", b"row stride 5")
    fails(lib.y3_export_rows(P, 1800, 6, P, 2, 300, 0, -1, 0, 0, 0, None, P, 600, P, None, 0, None), b"geometry", b"limit -1")
    fails(lib.y3_export_rows(P, 1800, 6, P, 2, 300, 3, 0, 0, 0, 0, None, P, 600, P, None, 0, None), b"form 3")
    fails(lib.y3_export_rows(P, 1800, 6, P, 2, 300, -1, 0, 0, 0, 0, None, P, 600, P, None, 0, None), b"form -1")
    fails(lib.y3_export_rows(P, 1800, 6, P, 2, 300, 1, 0, 0, 0, 0, None, P, 600, P, None, 0, None), b"txt", b"sizes")
    fails(lib.y3_export_rows(P, 1800, 6, None, 2, 300, 0, 0, 0, 0, 0, None, P, 599, P, None, 0, None), b"capacity 599", b"too small")
    fails(lib.y3_export_rows(P, 1800, 6, None, 2, 300, 0, 7, 0, 0, 0, None, P, 13, P, None, 0, None), b"capacity 13", b"2 x 7")
    fails(lib.y3_export_rows(P, 1800, 6, P, 2, 300, 0, 0, 0, 0, 0, None, P, -1, P, None, 0, None), b"capacity -1")
    fails(lib.y3_export_rows(P, 1800, 6, P, 2, 300, 0, 0, 0, 0, 0, None, P, 600, P, P, 0, None), b"histogram")


def test_ops_export_rows_has_no_cpu_path():
    from yolov3_amd import ops, outputs

    with pytest.raises(RuntimeError, match="no CPU"):
        ops.export_rows(torch.zeros(1, 2, 6), 12, 6, None, 1, 2, "target", 2)
    with pytest.raises(RuntimeError, match="no CPU"):
        outputs.save_txt_batched(torch.zeros(1, 2, 6), [2], [(4, 4)], ["a.jpg"], "unused")


def _files(lines, paths):
    return {f"{Path(p).stem}.txt": t.encode() for p, t in zip(paths, lines) if t}


@pytest.mark.parametrize("name", oc.TXT_CASES)
def test_txt_lines_of_the_golden_tables_are_the_reference_bytes(gold, name):
    from yolov3_amd import outputs

    g, c = gold["cases"][name], oc.case(name)
    for save_conf in (False, True):
        lines = outputs.txt_lines(g["txt"].numpy(), g["offsets"].numpy(), save_conf)
        assert len(lines) == len(c["counts"]) and _files(lines, c["paths"]) == g[f"files_conf{int(save_conf)}"], (name, save_conf)
        assert [bool(t) for t in lines] == [n > 0 for n in c["counts"]]   # no file for an image without detections
        if name == "detect":
            assert _files(outputs.txt_lines(g["detect"].numpy(), g["offsets"].numpy(), save_conf), c["paths"]) == g[f"detect_files_conf{int(save_conf)}"]
    text = b"".join(g["files_conf1"].values()).decode()
    assert "e-0" in text and re.search(r" 0\.\d+\n", text)   # %g in both of its forms


@pytest.mark.parametrize("name", oc.JSON_CASES)
def test_json_entries_of_the_golden_tables_are_the_reference_jdict(gold, name):
    from yolov3_amd import outputs

    g, c = gold["cases"][name], oc.case(name)
    class_map = outputs.coco80_to_coco91_class() if c["nc"] == 80 else list(range(1000))
    got = outputs.json_entries(g["json"].numpy(), g["offsets"].numpy(), c["paths"], class_map)
    assert got == g["jdict"] and len(got) == sum(c["counts"])
    assert {type(e["image_id"]) for e in got} == {int, str}   # numeric and non-numeric stems
    if name == "ids":
        assert max(e["category_id"] for e in got) == 364


@pytest.mark.parametrize("name", list(oc.CASES))
def test_host_path_of_cpu_tensors_reproduces_the_golden_tables(gold, name, tmp_path):
    """CPU detections never reach the kernel: the reference-signature functions then run the reference's tensor operations on the host"""
    from yolov3_amd import outputs

    g, c = gold["cases"][name], oc.case(name)
    dets = oc.dets(c)
    for limit in (c["limits"] or (300,)):
        got = outputs.output_to_target(dets, max_det=limit)
        assert got.dtype == np.float32 and np.array_equal(got, g[f"target_{limit}"].numpy()), (name, limit)
    for form, key, kw in (("txt", "txt", {}), ("json", "json", {}), ("txt", "detect", dict(round_boxes=True, reverse=True))):
        table, offs = outputs._list_table(dets, form, sizes0=c["shapes"], **kw)
        assert np.array_equal(table, g[key].numpy()) and np.array_equal(offs, g["offsets"].numpy()), (name, key)
    if name in oc.TXT_CASES:
        for d, shape, p in zip(dets, c["shapes"], c["paths"]):
            outputs.save_one_txt(d, True, shape, tmp_path / f"{Path(p).stem}.txt")
        assert {f.name: f.read_bytes() for f in sorted(tmp_path.iterdir())} == g["files_conf1"]
    if name in oc.JSON_CASES:
        jdict = []
        for d, p in zip(dets, c["paths"]):
            outputs.save_one_json(d, jdict, Path(p), oc.coco_map() if c["nc"] == 80 else list(range(1000)))
        assert jdict == g["jdict"]


def test_coco80_to_coco91_class():
    from yolov3_amd import coco80_to_coco91_class

    m = coco80_to_coco91_class()
    assert m == oc.coco_map() and len(m) == 80 and m == sorted(set(m)) and m[0] == 1 and m[-1] == 90 and not set(m) & set(oc.COCO_UNUSED_IDS)
    assert all(m[k] == v for k, v in oc.COCO_SPOT_CHECKS.items())


def _detections():
    from yolov3_amd import Detections

    c = oc.case("detect")
    ims = [np.zeros((*s, 3), np.uint8) for s in c["shapes"]]
    return Detections(ims, oc.dets(c), [Path(p).name for p in c["paths"]], oc.TIMES, dict(enumerate(oc.NAMES)), oc.DETECTIONS_SHAPE)


def test_detections_strings_on_cpu_tensors_equal_the_reference(gold, caplog):
    import logging

    d = _detections()
    assert str(d) == gold["detections"]["str"]
    assert repr(d) == gold["detections"]["repr"].replace("models.common.Detections", "yolov3_amd.autoshape.Detections")
    assert "(no detections)" in str(d) and re.search(r"\b2 class\d+s,", str(d)) and re.search(r"\b1 class\d+(,|\n)", str(d))
    with caplog.at_level(logging.INFO, logger="yolov3_amd"):
        d.print()
    assert str(d) in caplog.text


def test_detections_pandas_on_cpu_tensors_equals_the_reference(gold):
    frames = _detections().pandas()
    for k, want in gold["detections"]["pandas"].items():
        got = getattr(frames, k)
        assert len(got) == len(want)
        for df, (columns, values) in zip(got, want):
            assert list(df.columns) == columns and df.values.tolist() == values, k
    assert isinstance(_detections().xyxy[0], torch.Tensor)   # pandas() returns a copy


def test_run_batches_argument_errors_come_before_any_device_work(tmp_path):
    """no model is called and no stream is made: on a machine without a GPU anything later than the argument check raises something else"""
    from yolov3_amd import run_batches

    class Never:
        def __call__(self, *a, **k):
            raise AssertionError("the model was called")

    im, targets = torch.zeros(1, 3, 32, 32), torch.zeros(0, 6)
    shapes = [((32, 32), ((1.0, 1.0), (0.0, 0.0)))]
    for flags in (dict(save_txt=True), dict(save_json=True), dict(save_txt=True, save_conf=True, save_json="p.json")):
        with pytest.raises(ValueError, match="save_dir"):
            run_batches(Never(), [(im, targets, ["a.jpg"], shapes)], 80, **flags)
        with pytest.raises(ValueError, match="4-tuples"):
            run_batches(Never(), [(im, targets, shapes)], 80, save_dir=tmp_path / "run", **flags)
    assert not (tmp_path / "run").exists()
