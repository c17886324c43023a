"""CPU tests of the device-side autoanchor (csrc/autoanchor.hip, yolov3_amd/autoanchor.py): the public surface, the C ABI's argument validation without a GPU,
and the NumPy restatement of tests/autoanchor_cases.py against the fixtures of the unmodified reference (tests/golden/make_autoanchor_golden.py) -- and, where
the reference tree is readable, against the live reference."""
import re
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests"))

import autoanchor_cases as ac  # noqa: E402

NEW_SYMBOLS = ["y3_anchor_workspace_bytes", "y3_anchor_metrics", "y3_anchor_evolve", "y3_kmeans_step"]


@pytest.fixture(scope="module")
def lib():
    from yolov3_amd import _lib, build

    build.build(verbose=False)
    return _lib.lib()


@pytest.fixture(scope="module")
def gold(golden_dir):
    return torch.load(golden_dir / "autoanchor.pt", weights_only=True)   # data only


def test_public_names_import():
    import yolov3_amd
    from yolov3_amd import anchor_metrics, autoanchor, check_anchor_order, check_anchors, kmean_anchors, yolo

    assert autoanchor.check_anchors is check_anchors and autoanchor.kmean_anchors is kmean_anchors and autoanchor.anchor_metrics is anchor_metrics
    assert autoanchor.check_anchor_order is yolo.check_anchor_order is check_anchor_order and callable(yolov3_amd.check_anchors)
    from yolov3_amd import ops

    assert callable(ops.anchor_metrics) and callable(ops.anchor_evolve) and callable(ops.kmeans_step)


def test_new_symbols_are_declared_bound_and_exported_at_abi_6(lib):
    from yolov3_amd import _lib

    header = (ROOT / "include" / "yolov3_hip.h").read_text()
    declared = set(re.findall(r"\b(y3_[a-z0-9_]+)\s*\(", header))
    assert set(NEW_SYMBOLS) <= declared and set(NEW_SYMBOLS) <= set(_lib.exported_symbols())
    assert "#define Y3_ABI_VERSION 6" in re.sub(r"[ \t]+", " ", header) and lib.y3_abi_version() == 6 == _lib.ABI_VERSION
    assert ("autoanchor.hip", ["-ffp-contract=off"]) in __import__("yolov3_amd.build", fromlist=["SOURCES"]).SOURCES
    assert all(s in (ROOT / "INTEGRATION.md").read_text() for s in NEW_SYMBOLS)


def test_new_exports_reject_bad_arguments_without_a_gpu(lib):
    P = 1 << 20   # a fake, aligned device address: validation never dereferences it

    def fails(status, *needles):
        msg = lib.y3_last_error()
        assert status != 0 and all(n in msg for n in needles), (status, msg)

    big = lib.y3_anchor_workspace_bytes(860_000, 9, 30)
    small = lib.y3_anchor_workspace_bytes(312, 9, 0)
    assert small >= 256 + 2 * 6 * 8 and big >= 30 * 256 * 28 * 8 and big % 8 == 0 and small % 8 == 0
    for bad in ((0, 9, 0), (312, 0, 0), (312, 65, 0), (312, 9, 65), (312, 9, -1), (1 << 31, 9, 0)):
        assert lib.y3_anchor_workspace_bytes(*bad) == 0 and b"y3_anchor_workspace_bytes" in lib.y3_last_error() and b"geometry" in lib.y3_last_error()

    fails(lib.y3_anchor_metrics(None, 312, P, 9, 0.25, P, P, small, None), b"y3_anchor_metrics", b"null")
    fails(lib.y3_anchor_metrics(P, 312, P, 9, 0.25, None, P, small, None), b"y3_anchor_metrics", b"null")
    fails(lib.y3_anchor_metrics(P, 312, P, 65, 0.25, P, P, small, None), b"y3_anchor_metrics", b"65 anchors")
    fails(lib.y3_anchor_metrics(P, 312, P, 0, 0.25, P, P, small, None), b"y3_anchor_metrics", b"0 anchors")
    fails(lib.y3_anchor_metrics(P, 0, P, 9, 0.25, P, P, small, None), b"y3_anchor_metrics", b"label count")
    fails(lib.y3_anchor_metrics(P, 312, P + 4, 9, 0.25, P, P, small, None), b"y3_anchor_metrics", b"aligned")
    fails(lib.y3_anchor_metrics(P, 312, P, 9, 0.25, P + 4, P, small, None), b"y3_anchor_metrics", b"aligned")
    fails(lib.y3_anchor_metrics(P, 312, P, 9, 0.25, P, P, small - 1, None), b"y3_anchor_metrics", b"workspace needs")

    fails(lib.y3_anchor_evolve(P, 312, None, P, 9, P, 10, 0.25, P, P, small, None), b"y3_anchor_evolve", b"null")
    fails(lib.y3_anchor_evolve(P, 312, P, P, 9, None, 10, 0.25, P, P, small, None), b"y3_anchor_evolve", b"null")
    fails(lib.y3_anchor_evolve(P, 312, P, P, 9, P, 10, 0.25, None, P, small, None), b"y3_anchor_evolve", b"null")
    fails(lib.y3_anchor_evolve(P, 312, P, P, 9, P, -1, 0.25, P, P, small, None), b"y3_anchor_evolve", b"gen -1")
    fails(lib.y3_anchor_evolve(P, 312, P, P, 70, P, 10, 0.25, P, P, small, None), b"y3_anchor_evolve", b"70 anchors")
    fails(lib.y3_anchor_evolve(P, -5, P, P, 9, P, 10, 0.25, P, P, small, None), b"y3_anchor_evolve", b"label count")
    fails(lib.y3_anchor_evolve(P, 312, P, P + 4, 9, P, 10, 0.25, P, P, small, None), b"y3_anchor_evolve", b"aligned")
    fails(lib.y3_anchor_evolve(P, 312, P, P, 9, P + 2, 10, 0.25, P, P, small, None), b"y3_anchor_evolve", b"aligned")
    fails(lib.y3_anchor_evolve(P, 312, P, P, 9, P, 10, 0.25, P, P, 8, None), b"y3_anchor_evolve", b"workspace needs")

    km = lib.y3_anchor_workspace_bytes(312, 9, 30)
    fails(lib.y3_kmeans_step(P, 312, 9, 30, None, P, 0, P, P, km, None), b"y3_kmeans_step", b"null")
    fails(lib.y3_kmeans_step(P, 312, 9, 30, P, P, 0, None, P, km, None), b"y3_kmeans_step", b"null")
    fails(lib.y3_kmeans_step(P, 312, 0, 30, P, P, 0, P, P, km, None), b"y3_kmeans_step", b"0 codes")
    fails(lib.y3_kmeans_step(P, 312, 9, 65, P, P, 0, P, P, km, None), b"y3_kmeans_step", b"65 restarts")
    fails(lib.y3_kmeans_step(P, 312, 9, 0, P, P, 0, P, P, km, None), b"y3_kmeans_step", b"0 restarts")
    fails(lib.y3_kmeans_step(P, 0, 9, 30, P, P, 0, P, P, km, None), b"y3_kmeans_step", b"point count")
    fails(lib.y3_kmeans_step(P, 312, 9, 30, P + 4, P, 0, P, P, km, None), b"y3_kmeans_step", b"aligned")
    fails(lib.y3_kmeans_step(P, 312, 9, 30, P, P, 0, P, P, small, None), b"y3_kmeans_step", b"workspace needs")


def test_datasets_are_what_the_golden_was_made_from(gold):
    assert list(gold["cases"]) == list(ac.CASES)
    for name, g in gold["cases"].items():
        ds = ac.make_dataset(name)
        assert abs(ac.dataset_checksum(ds) - g["checksum"]) < 1e-6, f"{name}: the seeded dataset drifted"
        wh0 = ac.label_wh(ds, ac.IMG_SIZE)
        wh = wh0[(wh0 >= 2.0).any(1)].astype(np.float32)
        assert len(wh) == g["N"]
    N = {c: g["N"] for c, g in gold["cases"].items()}
    assert 256 < N["A"] < 512 and N["A"] % 64 and N["C"] > 4096 and N["C"] % 64 and N["D"] == 9 and N["E"] == 40
    assert gold["cases"]["E"]["fallback"] and gold["cases"]["E"]["book_rows"] < 9 and not any(gold["cases"][c]["fallback"] for c in "ABCD")
    for c in "ABCD":   # the generator's conditions: decisions and iteration counts are away from the rounding edges
        g = gold["cases"][c]
        assert g["margin"] >= 32 * g["meangap"]
        assert g["kmeans_gap"] <= 2e-6 and g["kmeans_min_gap"] > 1e-9 and g["kmeans_stop_edge"] > 1e-9


@pytest.mark.parametrize("case", list(ac.CASES))
def test_restatement_reproduces_the_golden(gold, case):
    g = gold["cases"][case]
    ds = ac.make_dataset(case)
    wh0 = ac.label_wh(ds, ac.IMG_SIZE)
    wh = wh0[(wh0 >= 2.0).any(1)].astype(np.float32)
    # the metric: counts exact, means within the fp32 summation error of the reference (values in [0, 1], cascade sum: (log2 N + 2) 2^-24 < 1e-6 for N <= 8192)
    for name, r in g["metrics"].items():
        m = ac.metrics(wh, r["k"].numpy())
        assert m["bpr"] == np.float32(r["bpr"]) and m["aat"] == np.float32(r["aat"]), name
        for key in ("fitness", "x_mean", "best_mean", "past_thr_mean"):
            assert abs(m[key] - float(r[key])) <= 2e-6 * abs(float(r[key])), (name, key, m[key], float(r[key]))
    # the genetic stage from the recorded k0 and v: decisions and anchors bit for bit
    got = ac.kmean_anchors(ds, n=g["n"], gen=g["gen"], init=g["k0"].numpy(), mutations=g["v"].numpy(), record=(rec := {}))
    assert np.array_equal(rec["accepted"], g["accepted"].numpy()) and np.array_equal(got, g["final"].numpy())
    assert np.abs(rec["fitness"] - g["fitness"].numpy()).max() <= 2e-6
    # k-means from the recorded index sets
    s = wh.std(0)
    book, d, iters = ac.kmeans(wh / s, g["index_sets"].numpy())
    assert np.array_equal(iters, g["kmeans_iters"].numpy()) and len(book) == g["book_rows"]
    if case != "E":
        assert np.abs(book - g["book"].numpy()).max() <= 1e-5 and abs(d - g["distortion"]) <= 1e-5
    # the whole procedure from the seed: the random streams are consumed as the reference consumes them
    ac.seed_all(g["seed"])
    whole = ac.kmean_anchors(ds, n=g["n"], gen=g["gen"], record=(rec := {}))
    assert np.array_equal(rec["v"], g["v"].numpy()) and np.array_equal(rec.get("index_sets"), g["index_sets"].numpy())
    assert np.abs(rec["k0"] - g["k0"].numpy()).max() <= 1e-5 * np.abs(g["k0"].numpy()).max() and whole.shape == (g["n"], 2) and whole.dtype == np.float32
    if case == "E":
        assert rec.get("fallback") and np.array_equal(whole, g["final"].numpy())   # the random init is exact: nothing of k-means enters it


def test_restatement_check_anchors_reproduces_the_golden(gold):
    ds = ac.make_dataset("A")
    for family, g in gold["check"].items():
        ac.seed_all(g["seed"])
        got = ac.check_anchors(ds, g["before"].numpy(), ac.ANCHORS[family][1], record=(rec := {}))
        want = g["after"].numpy()
        assert np.array_equal(rec["wh"], g["wh"].numpy()) and float(rec["bpr"]) == g["bpr"] <= 0.98 and float(rec["new_bpr"]) == g["new_bpr"] > g["bpr"]
        assert got.shape == want.shape and (np.abs(got - want) / np.abs(want)).max() <= 1e-5
        assert not np.array_equal(want, g["before"].numpy())


def test_restatement_reproduces_the_live_reference_on_case_a(gold):
    from oracle import ref_shim

    if not ref_shim.available():
        pytest.skip("the reference tree is not readable here")
    pytest.importorskip("scipy")
    sys.path.insert(0, str(ROOT / "tests" / "golden"))
    import make_autoanchor_golden as gen

    ra, vq = gen.reference()
    g = gold["cases"]["A"]
    ds = ac.make_dataset("A")
    rec = gen.run_reference_kmean(ra, vq, ds, g["n"], g["gen"], g["seed"])
    assert np.array_equal(rec["final"], g["final"].numpy()) and np.array_equal(rec["index_sets"], g["index_sets"].numpy())
    got = ac.kmean_anchors(ds, n=g["n"], gen=g["gen"], init=g["k0"].numpy(), mutations=g["v"].numpy())
    assert np.array_equal(got, rec["final"])
    book, d, _ = ac.kmeans(rec["obs"], rec["index_sets"])
    assert np.abs(book - rec["book"]).max() <= 1e-5


def test_kmean_anchors_refuses_a_yaml_path_and_cpu_inputs():
    from yolov3_amd import anchor_metrics, check_anchors, kmean_anchors

    with pytest.raises(NotImplementedError, match="yaml"):
        kmean_anchors("x.yaml")
    with pytest.raises(RuntimeError, match="no CPU"):
        anchor_metrics(torch.rand(10, 2) + 1, np.ones((3, 2)))
    import types

    m = types.SimpleNamespace(anchors=torch.ones(2, 3, 2), stride=torch.tensor([16.0, 32.0]))
    with pytest.raises(RuntimeError, match="no CPU"):
        check_anchors(ac.make_dataset("D"), types.SimpleNamespace(model=[m]))
