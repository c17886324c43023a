"""CPU tests of the device-side class / image weights (csrc/label_weights.hip, yolov3_amd/label_weights.py): the public surface, the C ABI's argument validation
without a GPU, the host tail of labels_to_class_weights, the dispatch on the argument's type, and the seeded cases against the fixtures of the unmodified
reference (tests/golden/make_label_weights_golden.py) -- and, where the reference tree is readable, against the live reference."""
import random
import re
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests"))

import label_weights_cases as lc  # noqa: E402

NEW_SYMBOLS = ["y3_label_histogram", "y3_image_weights", "y3_weighted_choices_workspace_bytes", "y3_weighted_choices"]


@pytest.fixture(scope="module")
def lib():
    from yolov3_amd import _lib, build

    build.build(verbose=False)
    return _lib.lib()


@pytest.fixture(scope="module")
def gold(golden_dir):
    return torch.load(golden_dir / "label_weights.pt", weights_only=True)   # data only


@pytest.fixture(scope="module")
def labels():
    return {c: lc.make_labels(c) for c in lc.CASES}


def test_public_names_import():
    import yolov3_amd
    from yolov3_amd import LabelTable, image_weight_indices, label_weights, labels_to_class_weights, labels_to_image_weights, ops

    assert label_weights.LabelTable is LabelTable and label_weights.labels_to_class_weights is labels_to_class_weights
    assert label_weights.labels_to_image_weights is labels_to_image_weights and label_weights.image_weight_indices is image_weight_indices
    assert callable(yolov3_amd.image_weight_indices) and callable(ops.label_histogram) and callable(ops.image_weights) and callable(ops.weighted_choices)


def test_new_symbols_are_declared_bound_and_exported_at_abi_6(lib):
    from yolov3_amd import _lib

    header = (ROOT / "include" / "yolov3_hip.h").read_text()
    declared = set(re.findall(r"\b(y3_[a-z0-9_]+)\s*\(", header))
    assert set(NEW_SYMBOLS) <= declared and set(NEW_SYMBOLS) <= set(_lib.exported_symbols()) and declared == set(_lib.exported_symbols())
    assert "#define Y3_ABI_VERSION 6" in re.sub(r"[ \t]+", " ", header) and lib.y3_abi_version() == 6 == _lib.ABI_VERSION
    assert ("label_weights.hip", ["-ffp-contract=off"]) in __import__("yolov3_amd.build", fromlist=["SOURCES"]).SOURCES
    assert all(s in (ROOT / "INTEGRATION.md").read_text() for s in NEW_SYMBOLS)
    source = (ROOT / "yolov3_amd" / "label_weights.py").read_text()
    assert "_lib" not in source and "ctypes" not in source   # the module marshals no C call itself
    assert not re.search(r"torch\.(bincount|cumsum|searchsorted|histc|bucketize|sum|multinomial)\b", source)   # no torch compute stands in for a kernel


def test_new_exports_reject_bad_arguments_without_a_gpu(lib):
    P = 1 << 20   # a fake, aligned device address: validation never dereferences it

    def fails(status, *needles):
        msg = lib.y3_last_error()
        assert status != 0 and all(n in msg for n in needles), (status, msg)

    fails(lib.y3_label_histogram(None, 1, 10, P, 80, None), b"y3_label_histogram", b"null")
    fails(lib.y3_label_histogram(P, 1, 10, None, 80, None), b"y3_label_histogram", b"null")
    fails(lib.y3_label_histogram(P, 1, -1, P, 80, None), b"y3_label_histogram", b"geometry")
    fails(lib.y3_label_histogram(P, 0, 10, P, 80, None), b"y3_label_histogram", b"geometry")
    fails(lib.y3_label_histogram(P, 1, 1 << 31, P, 80, None), b"y3_label_histogram", b"geometry")
    fails(lib.y3_label_histogram(P, 1, 10, P, 0, None), b"y3_label_histogram", b"0 classes")
    fails(lib.y3_label_histogram(P, 1, 10, P, 4097, None), b"y3_label_histogram", b"4097 classes")

    fails(lib.y3_image_weights(None, 10, P, 4, P, 80, P, None), b"y3_image_weights", b"null")
    fails(lib.y3_image_weights(P, 10, None, 4, P, 80, P, None), b"y3_image_weights", b"null")
    fails(lib.y3_image_weights(P, 10, P, 4, None, 80, P, None), b"y3_image_weights", b"null")
    fails(lib.y3_image_weights(P, 10, P, 4, P, 80, None, None), b"y3_image_weights", b"null")
    fails(lib.y3_image_weights(P, -1, P, 4, P, 80, P, None), b"y3_image_weights", b"geometry")
    fails(lib.y3_image_weights(P, 10, P, 0, P, 80, P, None), b"y3_image_weights", b"geometry")
    fails(lib.y3_image_weights(P, 10, P, -3, P, 80, P, None), b"y3_image_weights", b"geometry")
    fails(lib.y3_image_weights(P, 10, P, 4, P, 0, P, None), b"y3_image_weights", b"0 classes")
    fails(lib.y3_image_weights(P, 10, P + 4, 4, P, 80, P, None), b"y3_image_weights", b"aligned")
    fails(lib.y3_image_weights(P, 10, P, 4, P + 4, 80, P, None), b"y3_image_weights", b"aligned")
    fails(lib.y3_image_weights(P, 10, P, 4, P, 80, P + 4, None), b"y3_image_weights", b"aligned")

    assert lib.y3_weighted_choices_workspace_bytes(1) == 16 and lib.y3_weighted_choices_workspace_bytes(2048) == 2049 * 8
    assert lib.y3_weighted_choices_workspace_bytes(2049) == (2049 + 2) * 8 and lib.y3_weighted_choices_workspace_bytes(20_000) == (20_000 + 10) * 8
    for bad in (0, -1, 1 << 31):
        assert lib.y3_weighted_choices_workspace_bytes(bad) == 0 and b"y3_weighted_choices_workspace_bytes" in lib.y3_last_error() and b"geometry" in lib.y3_last_error()
    ws = lib.y3_weighted_choices_workspace_bytes(257)
    fails(lib.y3_weighted_choices(None, 257, P, 257, P, P, ws, None), b"y3_weighted_choices", b"null")
    fails(lib.y3_weighted_choices(P, 257, None, 257, P, P, ws, None), b"y3_weighted_choices", b"null")
    fails(lib.y3_weighted_choices(P, 257, P, 257, None, P, ws, None), b"y3_weighted_choices", b"null")
    fails(lib.y3_weighted_choices(P, 257, P, 257, P, None, ws, None), b"y3_weighted_choices", b"null")
    fails(lib.y3_weighted_choices(P, 0, P, 257, P, P, ws, None), b"y3_weighted_choices", b"geometry")
    fails(lib.y3_weighted_choices(P, 257, P, -1, P, P, ws, None), b"y3_weighted_choices", b"geometry")
    fails(lib.y3_weighted_choices(P + 4, 257, P, 257, P, P, ws, None), b"y3_weighted_choices", b"aligned")
    fails(lib.y3_weighted_choices(P, 257, P, 257, P + 4, P, ws, None), b"y3_weighted_choices", b"aligned")
    fails(lib.y3_weighted_choices(P, 257, P, 257, P, P, ws - 1, None), b"y3_weighted_choices", b"workspace needs")


def test_case_builders_reproduce_the_golden(gold, labels):
    assert list(gold["cases"]) == list(lc.CASES)
    for name, g in gold["cases"].items():
        lb = labels[name]
        assert abs(lc.checksum(lb) - g["checksum"]) < 1e-6, f"{name}: the seeded labels drifted"
        assert len(lb) == g["n"] == lc.CASES[name]["n_img"] and sum(len(l) for l in lb) == g["N"] and all(l.dtype == np.float32 and l.shape[1] == 5 for l in lb)
        assert np.array_equal(lc.make_maps(name), g["maps"].numpy())
    a, d = labels["A"], labels["D"]
    assert len(a[0]) == 0 and len(a[-1]) == 0 and max(len(l) for l in a) <= 40 and gold["cases"]["A"]["N"] % 64 and any((l[:, 0] % 1 > 0.5).any() for l in a)
    assert len(d[7]) == 5000 and sum(len(l) == 0 for l in d) == 10
    assert len(np.unique(lc.class_ids(labels["C"]))) == 40 and gold["cases"]["E"]["N"] == 0 and 140_000 < gold["cases"]["F"]["N"] < 160_000
    for name in "ABCDF":   # the generator's condition: no draw near a boundary
        g = gold["cases"][name]
        assert g["margin"] >= lc.MARGIN and 0 <= g["seed"] < 32
        random.seed(g["seed"])
        k = 3 * g["n"] if name == "A" else g["n"]
        assert abs(lc.boundary_margin(g["iw"].numpy(), [random.random() for _ in range(k)]) - g["margin"]) <= 1e-15
    assert gold["cases"]["E"]["seed"] == -1 and not gold["cases"]["E"]["iw"].any()


def _table_of(case_labels, nc):
    """a LabelTable as its constructor leaves it, minus the device buffers: what the host-side code paths read"""
    from yolov3_amd import LabelTable

    t = object.__new__(LabelTable)
    t.nc, t.n, t.N, t.device = nc, len(case_labels), sum(len(l) for l in case_labels), torch.device("cpu")
    t._counts = np.bincount(lc.class_ids(case_labels), minlength=nc).astype(np.int64) if t.N else np.zeros(nc, dtype=np.int64)
    t.cls, t.offsets = torch.zeros(t.N), torch.zeros(t.n + 1, dtype=torch.int64)
    return t


@pytest.mark.parametrize("case", list(lc.CASES))
def test_host_tail_of_class_weights_is_the_reference_bit_for_bit(gold, labels, case):
    from yolov3_amd import labels_to_class_weights

    g = gold["cases"][case]
    got = labels_to_class_weights(_table_of(labels[case], g["nc"]), nc=g["nc"])
    assert got.dtype == torch.float32 and got.device.type == "cpu" and torch.equal(got, g["class_weights"])
    if case == "E":
        assert torch.equal(got, torch.full((80,), 1 / 80))


def test_dispatch_on_the_argument(labels):
    from yolov3_amd import LabelTable, image_weight_indices, labels_to_class_weights, labels_to_image_weights

    none = labels_to_class_weights([None, None], 80)   # no labels loaded: the reference's empty tensor, no device needed
    assert isinstance(none, torch.Tensor) and none.numel() == 0 and none.dtype == torch.float32
    if not torch.cuda.is_available():   # a list needs a device
        with pytest.raises(RuntimeError, match="no CPU"):
            labels_to_class_weights(labels["B"], 1)
        with pytest.raises(RuntimeError, match="no CPU"):
            labels_to_image_weights(labels["B"], 1, np.ones(1))
        with pytest.raises(RuntimeError, match="no CPU"):
            LabelTable(labels["B"], 1)
    for call in (lambda: LabelTable(labels["B"], 1, "cpu"), lambda: labels_to_class_weights(labels["B"], 1, device="cpu"),
                 lambda: labels_to_image_weights(labels["B"], 1, np.ones(1), device="cpu")):
        with pytest.raises(RuntimeError, match="no CPU"):
            call()
    # a table is used as it is: its buffers go to the kernels (refused here: they are CPU tensors), its nc decides
    t = _table_of(labels["A"], 80)
    with pytest.raises(RuntimeError, match="no CPU"):
        labels_to_image_weights(t, 80, np.ones(80))
    with pytest.raises(ValueError):
        labels_to_image_weights(t, 80, np.ones(81))
    with pytest.raises(ValueError, match="finite"):
        labels_to_image_weights(t, 80, np.full(80, np.inf))
    state = random.getstate()
    with pytest.raises(ValueError, match="finite"):
        image_weight_indices(t, np.full(80, np.nan))
    with pytest.raises(TypeError, match="LabelTable"):
        image_weight_indices(labels["A"], np.ones(80))
    assert random.getstate() == state


def test_cpu_tensors_are_refused():
    from yolov3_amd import ops

    with pytest.raises(RuntimeError, match="no CPU"):
        ops.label_histogram(torch.zeros(10), 80)
    with pytest.raises(RuntimeError, match="no CPU"):
        ops.image_weights(torch.zeros(10), torch.zeros(3, dtype=torch.int64), torch.ones(80, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="no CPU"):
        ops.weighted_choices(torch.ones(10, dtype=torch.float64), torch.rand(10, dtype=torch.float64))


@pytest.mark.parametrize("case", ["A", "C", "D", "E"])
def test_golden_is_what_the_live_reference_computes(gold, labels, case):
    from oracle import ref_shim

    if not ref_shim.available():
        pytest.skip("the reference tree is not readable here")
    sys.path.insert(0, str(ROOT / "tests" / "golden"))
    import make_label_weights_golden as gen

    g = gold["cases"][case]
    state = random.getstate()
    live = gen.run_case(*gen.reference(), case)
    random.setstate(state)
    assert torch.equal(live["class_weights"], g["class_weights"]) and torch.equal(live["cw"], g["cw"]) and torch.equal(live["iw"], g["iw"]) and live["seed"] == g["seed"]
    if case != "E":
        assert torch.equal(live["indices"], g["indices"]) and live["next_random"] == g["next_random"]
