"""GPU tests of the device-side class / image weights (csrc/label_weights.hip through yolov3_amd/label_weights.py) against the fixtures of the unmodified reference
(tests/golden/label_weights.pt, made by tests/golden/make_label_weights_golden.py).  Cases: tests/label_weights_cases.py."""
import random
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests"))

import label_weights_cases as lc  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
IW_RTOL = 1e-12   # two summation orders of at most nc + m non-negative terms differ by at most 2 (nc + m) 2^-53 relative: below 1.2e-12 for nc + m < 5400 (case D: 80 + 5000)


@pytest.fixture(scope="module")
def gold(golden_dir):
    return torch.load(golden_dir / "label_weights.pt", weights_only=True)   # data only


@pytest.fixture(scope="module")
def labels():
    return {c: lc.make_labels(c) for c in lc.CASES}


@pytest.fixture(scope="module")
def tables(labels):
    """case -> LabelTable, uploaded once"""
    from yolov3_amd import LabelTable

    return {c: LabelTable(labels[c], lc.CASES[c]["nc"], DEV) for c in lc.CASES}


@pytest.mark.parametrize("case", ["A", "B", "C", "D", "E"])
def test_class_weights_are_the_reference_bit_for_bit(gold, labels, tables, case):
    from yolov3_amd import labels_to_class_weights

    g, t = gold["cases"][case], tables[case]
    assert (t.n, t.N, t.nc) == (g["n"], g["N"], g["nc"]) and t.cls.dtype == torch.float32 and t.cls.is_contiguous() and tuple(t.offsets.shape) == (t.n + 1,)
    counts = t.class_counts()
    want = np.bincount(lc.class_ids(labels[case]), minlength=g["nc"]) if g["N"] else np.zeros(g["nc"], dtype=np.int64)
    assert counts.dtype == np.int64 and np.array_equal(counts, want)
    got = labels_to_class_weights(t, g["nc"])
    assert got.dtype == torch.float32 and got.device.type == "cpu" and torch.equal(got, g["class_weights"])
    if case in "BE":   # the list form builds its own table on the given device
        assert torch.equal(labels_to_class_weights(labels[case], g["nc"], device=DEV), g["class_weights"])


@pytest.mark.parametrize("case", ["A", "B", "C", "D", "E", "F"])
def test_image_weights_match_the_reference(gold, labels, tables, case):
    from yolov3_amd import labels_to_image_weights

    g = gold["cases"][case]
    iw = labels_to_image_weights(tables[case], g["nc"], g["cw"].numpy())
    ref = g["iw"].numpy()
    err = np.abs(iw - ref)
    print(case, "largest relative gap", float((err[ref > 0] / ref[ref > 0]).max()) if (ref > 0).any() else 0.0)
    assert iw.dtype == np.float64 and iw.shape == (g["n"],)
    assert (err <= IW_RTOL * ref).all()
    empty = np.array([len(l) == 0 for l in labels[case]])
    assert empty.any() and (iw[empty] == 0.0).all() and (empty.all() if case == "E" else (iw[~empty] > 0.0).all())
    # weights of 1: sums of small integers are exact in any order
    ones = labels_to_image_weights(tables[case], g["nc"], np.ones(g["nc"]))
    assert np.array_equal(ones, g["iw_ones"].numpy()) and np.array_equal(ones, np.array([len(l) for l in labels[case]], dtype=np.float64))
    if case == "D":   # the default argument (nc = 80, ones) and the list form
        assert np.array_equal(labels_to_image_weights(tables[case]), ones) and np.array_equal(labels_to_image_weights(labels[case], 80, g["cw"].numpy(), device=DEV), iw)


@pytest.mark.parametrize("case", ["A", "B", "C", "D", "F"])
def test_indices_are_the_reference_draw(gold, tables, case):
    from yolov3_amd import image_weight_indices

    g, t = gold["cases"][case], tables[case]
    random.seed(g["seed"])
    got, iw = image_weight_indices(t, g["cw"].numpy(), device_weights=True)
    after = random.random()
    want = g["indices"].tolist()
    print(case, "seed", g["seed"], "margin", g["margin"], "differing", sum(a != b for a, b in zip(got, want)))
    assert isinstance(got, list) and len(got) == t.n and all(type(i) is int for i in got[:8]) and got == want
    assert after == g["next_random"]   # the stream is where the reference leaves it
    assert iw.is_cuda and iw.dtype == torch.float64 and (np.abs(iw.cpu().numpy() - g["iw"].numpy()) <= IW_RTOL * g["iw"].numpy()).all()
    if case == "A":
        random.seed(g["seed"])
        second = random.Random(g["seed"])
        second.random()
        assert image_weight_indices(t, g["cw"].numpy(), k=1) == want[:1] and random.random() == second.random()
        random.seed(g["seed"])
        assert image_weight_indices(t, g["cw"].numpy(), k=3 * t.n) == g["indices_3n"].tolist() and random.random() == g["next_random_3n"]
        random.seed(g["seed"])
        assert image_weight_indices(t, g["cw"].numpy(), k=0) == [] and random.random() == random.Random(g["seed"]).random()


def test_zero_total_raises_and_leaves_the_stream_alone(gold, tables):
    from yolov3_amd import image_weight_indices, labels_to_class_weights

    g, t = gold["cases"]["E"], tables["E"]
    assert torch.equal(labels_to_class_weights(t, 80), torch.full((80,), 1 / 80))
    random.seed(5)
    state = random.getstate()
    with pytest.raises(ValueError, match="Total of weights must be greater than zero"):
        image_weight_indices(t, g["cw"].numpy())
    assert random.getstate() == state
    with pytest.raises(ValueError, match="Total of weights must be greater than zero"):   # a negative total on labelled images, as random.choices judges it
        image_weight_indices(tables["B"], np.array([-1.0]))
    assert random.getstate() == state


def test_refusals(labels, tables):
    from yolov3_amd import LabelTable, image_weight_indices, labels_to_image_weights

    def with_id(v):
        lb = [l.copy() for l in labels["A"][:9]]
        next(l for l in lb if len(l) >= 3)[2, 0] = v
        return lb

    for bad in (80.0, 80.9, -1.5, -1.0, float("nan"), 1e10):
        with pytest.raises(ValueError, match="outside"):
            LabelTable(with_id(bad), 80, DEV)
    for ok, cls in ((-0.5, 0), (79.9, 79), (-0.0, 0)):   # astype(int) truncates toward zero
        t = LabelTable(with_id(ok), 80, DEV)
        want = np.bincount(lc.class_ids(with_id(ok)), minlength=80)
        assert np.array_equal(t.class_counts(), want) and int(np.float32(ok)) == cls
    for bad in (np.inf, -np.inf, np.nan):
        cw = np.ones(80)
        cw[17] = bad
        state = random.getstate()
        with pytest.raises(ValueError, match="finite"):
            image_weight_indices(tables["A"], cw)
        with pytest.raises(ValueError, match="finite"):
            labels_to_image_weights(tables["A"], 80, cw)
        assert random.getstate() == state
    with pytest.raises(ValueError):
        LabelTable([], 80, DEV)
    f64 = [l.astype(np.float64) for l in labels["A"]]   # other dtypes truncate in their own precision
    f64[5][0, 0] = 2.9999999999
    assert np.array_equal(LabelTable(f64, 80, DEV).class_counts(), np.bincount(lc.class_ids(f64), minlength=80))


def test_every_call_is_bit_identical_run_to_run(gold, labels, tables):
    from yolov3_amd import LabelTable, image_weight_indices, labels_to_class_weights, labels_to_image_weights

    g, t = gold["cases"]["F"], tables["F"]
    t2 = LabelTable(labels["F"], 80, DEV)
    assert torch.equal(t.cls, t2.cls) and torch.equal(t.offsets, t2.offsets) and np.array_equal(t.class_counts(), t2.class_counts())
    assert torch.equal(labels_to_class_weights(t), labels_to_class_weights(t2))
    cw = g["cw"].numpy()
    runs = []
    for table in (t, t2, t):
        random.seed(11)   # (no golden seed: whatever a draw near a boundary gives, it gives again)
        idx, iw = image_weight_indices(table, cw, device_weights=True)
        runs.append((idx, iw.cpu().numpy(), labels_to_image_weights(table, 80, cw)))
    for idx, iw, iw_host in runs[1:]:
        assert idx == runs[0][0] and np.array_equal(iw, runs[0][1]) and np.array_equal(iw_host, runs[0][2]) and np.array_equal(iw, iw_host)


def test_epoch_call_traffic_is_two_uploads_two_launches_one_download(gold, tables, monkeypatch):
    from yolov3_amd import image_weight_indices, ops

    g, t = gold["cases"]["A"], tables["A"]
    cw = g["cw"].numpy()
    log = []
    for name in ("image_weights", "weighted_choices", "label_histogram"):
        real = getattr(ops, name)
        monkeypatch.setattr(ops, name, lambda *a, _real=real, _name=name, **k: (log.append(_name), _real(*a, **k))[1])
    for name in ("cpu", "item", "tolist", "numpy", "to", "cuda", "__getitem__", "sum", "cumsum"):
        orig = getattr(torch.Tensor, name)

        def counted(self, *a, _orig=orig, _name=name, **k):
            out = _orig(self, *a, **k)
            if _name in ("to", "cuda") and isinstance(out, torch.Tensor) and out.is_cuda and not self.is_cuda:
                log.append(("upload", self.numel() * self.element_size()))
            elif self.is_cuda:
                log.append((_name, self.numel() * self.element_size()))
            return out

        monkeypatch.setattr(torch.Tensor, name, counted)
    random.seed(g["seed"])
    got = image_weight_indices(t, cw)
    monkeypatch.undo()
    assert log == [("upload", 80 * 8), ("upload", t.n * 8), "image_weights", "weighted_choices", ("cpu", (t.n + 1) * 8)], log
    assert got == g["indices"].tolist()


def test_paths_the_cases_do_not_reach():
    """Sizes at which the kernels take another path, on synthetic integer data whose sums are exact in every order (so NumPy is an exact yardstick): one scan chunk
    (n <= 2048: no carry kernels), the chunk's edge, more than 256 chunks (the carry kernel's second tile), n = 1 (hi = 0), k = 0; the histogram's and the image
    kernel's grid-stride loops (more than 1024 x 256 labels, more than 65 536 x 4 images); the status words of a total that is zero, negative, infinite or NaN."""
    from yolov3_amd import ops

    rs = np.random.RandomState(3)
    for n in (1, 2, 2047, 2048, 2049, 256 * 2048 + 5):
        w = rs.randint(0, 9, n).astype(np.float64)
        w[rs.randint(0, n)] += 1.0
        u = np.concatenate([rs.random_sample(509), [0.0, 1.0 - 2.0 ** -53]])
        out = ops.weighted_choices(torch.from_numpy(w).to(DEV), torch.from_numpy(u).to(DEV)).cpu().numpy()
        cum = np.cumsum(w)
        want = np.minimum(np.searchsorted(cum, u * cum[-1], side="right"), n - 1)
        assert out[-1] == 0 and np.array_equal(out[:-1], want), n
    none = ops.weighted_choices(torch.ones(5, dtype=torch.float64, device=DEV), torch.zeros(0, dtype=torch.float64, device=DEV)).cpu().tolist()
    assert none == [0]
    u = torch.rand(3, dtype=torch.float64).to(DEV)
    for w, status in (([0.0, 0.0], 1), ([1.0, -2.0], 1), ([1.0, np.inf], 2), ([np.nan, 1.0], 2), ([np.inf, -np.inf], 2), ([-np.inf, 1.0], 1)):
        out = ops.weighted_choices(torch.tensor(w, dtype=torch.float64, device=DEV), u).cpu().tolist()
        assert out[-1] == status and all(0 <= i <= 1 for i in out[:-1]), (w, out)

    N, nc = 300_001, 365
    ids = rs.randint(0, nc, N)
    cls = torch.from_numpy((ids + rs.uniform(0.0, 0.9, N)).astype(np.float32)).to(DEV)
    assert np.array_equal(ops.label_histogram(cls, nc).cpu().numpy(), np.append(np.bincount(ids, minlength=nc), 0))
    assert np.array_equal(ops.label_histogram(cls, 100).cpu().numpy(), np.append(np.bincount(ids, minlength=nc)[:100], (ids >= 100).sum()))
    assert ops.label_histogram(cls[:0], 7).cpu().tolist() == [0] * 8
    cw = rs.randint(1, 50, nc).astype(np.float64)
    offsets = torch.arange(N + 1, dtype=torch.int64).to(DEV)   # one label per image
    iw = ops.image_weights(cls, offsets, torch.from_numpy(cw).to(DEV)).cpu().numpy()
    assert np.array_equal(iw, cw[ids])
    two = ops.image_weights(cls, torch.tensor([0, 70_000, N], dtype=torch.int64).to(DEV), torch.from_numpy(cw).to(DEV)).cpu().numpy()   # two very long segments
    assert np.array_equal(two, [cw[ids[:70_000]].sum(), cw[ids[70_000:]].sum()])
