"""CPU tests of the device-side validation statistics (csrc/val_stats.hip, yolov3_amd.metrics.ValStats / ConfusionMatrix / ap_per_class_device,
yolov3_amd.val.run_batches): the public surface, the C ABI's argument validation without a GPU, and the host mirror that states the tie rule."""
import ctypes as C
import re
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests"))

import val_stats_cases as vc  # noqa: E402

NEW_SYMBOLS = ["y3_val_stats_append", "y3_val_stats_count_labels", "y3_val_stats_out_elems", "y3_val_stats_workspace_bytes", "y3_val_stats_compute", "y3_confusion_matrix",
               "y3_labels_to_native"]


@pytest.fixture(scope="module")
def lib():
    from yolov3_amd import _lib, build

    build.build(verbose=False)
    return _lib.lib()


def test_public_names_import():
    import yolov3_amd
    from yolov3_amd import ConfusionMatrix, ValStats, ap_per_class_device, metrics, run_batches, val

    assert metrics.ValStats is ValStats and metrics.ConfusionMatrix is ConfusionMatrix and metrics.ap_per_class_device is ap_per_class_device
    assert val.run_batches is run_batches and callable(yolov3_amd.run_batches)
    cm = ConfusionMatrix(3)
    assert (cm.nc, cm.conf, cm.iou_thres) == (3, 0.25, 0.45) and cm.matrix.shape == (4, 4) and cm.matrix.dtype == np.float64
    with pytest.raises(NotImplementedError):
        cm.plot()


def test_new_symbols_are_declared_bound_and_exported_at_abi_5(lib):
    from yolov3_amd import _lib

    header = (ROOT / "include" / "yolov3_hip.h").read_text()
    declared = set(re.findall(r"\b(y3_[a-z0-9_]+)\s*\(", header))
    assert set(NEW_SYMBOLS) <= declared and set(NEW_SYMBOLS) <= set(_lib.exported_symbols())
    assert "#define Y3_ABI_VERSION 6" in re.sub(r"[ \t]+", " ", header) and lib.y3_abi_version() == 6 == _lib.ABI_VERSION
    assert ("val_stats.hip", ["-ffp-contract=off"]) in __import__("yolov3_amd.build", fromlist=["SOURCES"]).SOURCES


def test_new_exports_reject_bad_arguments_without_a_gpu(lib):
    P = 1 << 20   # a fake, aligned device address: validation never dereferences it

    def fails(status, *needles):
        msg = lib.y3_last_error()
        assert status != 0 and all(n in msg for n in needles), (status, msg)

    fails(lib.y3_val_stats_append(None, P, 1800, 6, P, 2, 300, P, 10, P, P, P, 0, 600, None), b"y3_val_stats_append", b"null")
    fails(lib.y3_val_stats_append(P, P, 1800, 6, P, 2, 300, P, 17, P, P, P, 0, 600, None), b"y3_val_stats_append", b"17")
    fails(lib.y3_val_stats_append(P, P, 1800, 6, P, 2, 300, P, 10, P, P, P, 700, 600, None), b"y3_val_stats_append", b"capacity")
    fails(lib.y3_val_stats_append(P, P, 1800, 6, None, 2, 300, P, 10, P, P, P, 100, 600, None), b"y3_val_stats_append", b"do not fit")
    fails(lib.y3_val_stats_append(P, P, 1800, 0, P, 2, 300, P, 10, P, P, P, 0, 600, None), b"y3_val_stats_append", b"geometry")
    fails(lib.y3_val_stats_count_labels(P, 5, 10, None, 80, None), b"y3_val_stats_count_labels", b"null")
    fails(lib.y3_val_stats_count_labels(P, 0, 10, P, 80, None), b"y3_val_stats_count_labels", b"geometry")
    assert lib.y3_val_stats_out_elems(80, 10) == 4 + 80 * 16 and lib.y3_val_stats_out_elems(0, 10) == 0
    small, big = lib.y3_val_stats_workspace_bytes(1000, 80), lib.y3_val_stats_workspace_bytes(1_500_000, 80)
    assert small >= 2 * 80 * 1000 * 8 and big >= small + 1_499_000 * (8 + 8 + 4 + 4 + 4 + 2)
    assert lib.y3_val_stats_workspace_bytes(-1, 80) == 0 and b"y3_val_stats_workspace_bytes" in lib.y3_last_error()
    n_out = lib.y3_val_stats_out_elems(80, 10)
    fails(lib.y3_val_stats_compute(P, P, P, 1000, None, 80, 10, 1e-16, P, P, P, n_out, P, small, None), b"y3_val_stats_compute", b"null")
    fails(lib.y3_val_stats_compute(None, P, P, 1000, P, 80, 10, 1e-16, P, P, P, n_out, P, small, None), b"y3_val_stats_compute", b"null rows")
    fails(lib.y3_val_stats_compute(P, P, P, 1000, P, 80, 0, 1e-16, P, P, P, n_out, P, small, None), b"y3_val_stats_compute", b"thresholds")
    fails(lib.y3_val_stats_compute(P, P, P, 1000, P, 80, 10, 1e-16, P, P, P, n_out - 1, P, small, None), b"y3_val_stats_compute", b"doubles")
    fails(lib.y3_val_stats_compute(P, P, P, 1000, P, 80, 10, 1e-16, P, P, P, n_out, P, small - 1, None), b"y3_val_stats_compute", b"workspace")
    fails(lib.y3_val_stats_compute(P, P, P, 1000, P, 80, 10, 1e-16, P, P, P, n_out, P + 8, small, None), b"y3_val_stats_compute", b"aligned")
    fails(lib.y3_confusion_matrix(P, 1800, 6, P, 2, 300, P, 5, None, 80, 0.25, 0.45, P, None), b"y3_confusion_matrix", b"null")
    fails(lib.y3_confusion_matrix(P, 1800, 6, P, 2, 5000, P, 5, P, 80, 0.25, 0.45, P, None), b"y3_confusion_matrix", b"max_det 5000")
    fails(lib.y3_confusion_matrix(P, 1800, 5, P, 2, 300, P, 5, P, 80, 0.25, 0.45, P, None), b"y3_confusion_matrix", b"strides")
    fails(lib.y3_confusion_matrix(None, 0, 6, None, 1, 300, P, 1, P, 80, 0.25, 0.45, P, None), b"y3_confusion_matrix", b"strides")
    fails(lib.y3_labels_to_native(P, 10, 2, 640.0, 640.0, P, P, None, None), b"y3_labels_to_native", b"null")
    fails(lib.y3_labels_to_native(P, 10, 2, 0.0, 640.0, P, P, P, None), b"y3_labels_to_native", b"geometry")


def _tuple_close(got, want, tol=1e-12):
    assert len(got) == len(want) == 7
    for i, (a, b) in enumerate(zip(got, want)):
        a, b = np.asarray(a), np.asarray(b)
        assert a.shape == b.shape, (i, a.shape, b.shape)
        if i in (0, 1, 6):
            assert np.array_equal(a, b), i        # integer counts and class ids: exact
        else:
            assert float(np.abs(a - b).max(initial=0.0)) <= tol, (i, float(np.abs(a - b).max()))


def test_stable_ranking_equals_the_default_on_tie_free_goldens(golden_dir):
    """the fixtures of the unmodified reference (tests/golden/make_val_stats_golden.py) have pairwise distinct confidences: both rankings of the host
    mirror agree with each other exactly and with the reference within 1e-12"""
    from yolov3_amd import metrics

    gold = torch.load(golden_dir / "val_stats.pt")["ap"]
    assert list(gold) == vc.AP_CASES
    for name in vc.AP_CASES:
        tp, conf, pc, tc = vc.ap_case(name)
        assert abs(float(tp.sum() + conf.astype(np.float64).sum() + pc.sum() + tc.sum()) - gold[name]["in_sum"]) < 1e-6, f"{name}: the seeded inputs drifted"
        assert len(np.unique(conf)) == conf.shape[0]
        plain, stable = metrics.ap_per_class(tp, conf, pc, tc), metrics.ap_per_class(tp, conf, pc, tc, stable=True)
        for a, b in zip(plain, stable):
            assert np.array_equal(a, b)
        _tuple_close(stable, [t.numpy() for t in gold[name]["out"]])
    tp, conf, pc, tc = vc.tied_ap_case()
    assert len(np.unique(conf)) < conf.shape[0] // 4   # the tie case really ties
    res = metrics.ap_per_class(tp, conf, pc, tc, stable=True)
    assert res[5].shape == (9, 10) and 0.0 < float(res[5].mean()) < 1.0


def test_device_statistics_refuse_cpu_tensors():
    from yolov3_amd import metrics

    with pytest.raises(RuntimeError, match="no CPU"):
        metrics.ValStats(80, torch.linspace(0.5, 0.95, 10), "cpu")
    with pytest.raises(RuntimeError, match="no CPU"):
        metrics.ap_per_class_device(torch.zeros(4, 10, dtype=torch.bool), torch.rand(4), torch.zeros(4), torch.zeros(3))
    cm = metrics.ConfusionMatrix(3)
    with pytest.raises(RuntimeError, match="no CPU"):
        cm.process_batch(torch.zeros(2, 6), torch.zeros(1, 5))
    with pytest.raises(RuntimeError, match="no CPU"):
        cm.process_batch(None, torch.zeros(2))
    with pytest.raises(RuntimeError, match="no CPU"):
        cm.process_batch_batched(torch.zeros(1, 3, 6), None, torch.zeros(1, 5), torch.tensor([0, 1]))


def test_confusion_inputs_cover_the_edge_cases(golden_dir):
    """the seeded image sequence still is what the fixture was generated from, and holds every edge case the issue lists"""
    gold = torch.load(golden_dir / "val_stats.pt")["confusion"]
    imgs = vc.confusion_images()
    assert abs(sum(float(d.double().abs().sum() + l.double().abs().sum()) for d, l in imgs) - gold["in_sum"]) < 1e-6
    assert any(d.shape[0] == 0 and l.shape[0] for d, l in imgs) and any(l.shape[0] == 0 and d.shape[0] for d, l in imgs)
    assert any(d.shape[0] and bool((d[:, 4] <= gold["conf"]).all()) for d, l in imgs)
    m = gold["matrix"].numpy()
    assert m.shape == (gold["nc"] + 1, gold["nc"] + 1) and m[-1, -1] == 0 and m[:, :-1].sum() == sum(l.shape[0] for d, l in imgs)   # every label lands in exactly one cell
