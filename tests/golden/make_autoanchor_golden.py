"""Generate tests/golden/autoanchor.pt from the UNMODIFIED reference (utils/autoanchor.py through oracle/ref_shim.py, scipy.cluster.vq.kmeans behind it).

    python tests/golden/make_autoanchor_golden.py

Only where the reference tree and scipy are present.  The file holds data only: per case the seed and the dataset's checksum (the dataset and both tables of
label sizes are rebuilt from the seed by tests/autoanchor_cases.py and checked against the checksum and N: storing them would store the builder's output
twice), the 30 initial index sets, scipy's codebook and distortion, the restatement's per-restart iteration
counts, k0, the mutations v, the reference's fp32 fitness of every generation, the accepted mask, the final anchors, bpr / aat of several anchor sets and
m.anchors before / after check_anchors for the yolov3 and yolov3-tiny strides.

Two traps of the shim are handled here: its TQDM stub iterates over nothing (kmean_anchors would run zero generations: utils.autoanchor.TQDM is replaced by a
pass-through at run time), and its TryExcept swallows exceptions (so the generator asserts that check_anchors really changed the anchors).

The datasets are fixed (tests/autoanchor_cases.py::CASES); for every case the first seed of the random streams in 0..31 is taken that satisfies all of:
  1. the restatement's genetic stage, from the reference's k0 and v, ends in the reference's anchors bit for bit;
  2. min over generations of |fg - f| / f is at least 32x the largest relative gap between the reference's fp32 mean and the fp64 mean: summation order
     cannot flip a decision;
  3. no k-means iteration of any restart has a change of the mean distance within 1e-9 of the stopping threshold 1e-5, and the nearest and second nearest
     code of every point differ by more than 1e-9 relative at every iteration.  The counts recorded are the fp64 restatement's and the device runs fp64 too, so
     the two can part only through summation order (1e-15 relative): 1e-9 leaves six orders of magnitude.  The measured minima go into the golden.  (A band of
     [0.5e-5, 2e-5] around the threshold and a gap of 1e-4 cannot be had with 30 restarts: Lloyd's iterations creep through that band on the way to the stop,
     10 to 15 iterations per case lie inside it, and among some 140 000 point-iterations the closest call is about 1e-5.)  Not for E, whose codes coincide by
     design.  The restatement's codebook lies within 2e-6 of scipy's fp32 one (measured: up to 1.9e-6, case C; the tests allow 1e-5);
  4. (check_anchors) the restatement's whole pipeline, k-means in fp64 included, ends within 1e-6 relative of the reference's anchors.
"""
import random
import sys
import types
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import autoanchor_cases as ac  # noqa: E402
from oracle import ref_shim  # noqa: E402


MARGIN_FACTOR = 32   # condition 2
EDGE_MIN, GAP_MIN = 1e-9, 1e-9   # condition 3


class _Pbar:
    def __init__(self, it):
        self.it, self.desc = it, ""

    def __iter__(self):
        return iter(self.it)


def reference():
    ref_shim.install()
    import scipy.cluster.vq as vq
    import utils.autoanchor as ra  # type: ignore

    ra.TQDM = _Pbar
    return ra, vq


def ref_fitness32(wh, k, thr):
    """anchor_fitness exactly as the reference forms it (fp32 tensors, fp32 mean) plus the same mean in fp64"""
    wh = torch.tensor(wh, dtype=torch.float32)
    r = wh[:, None] / torch.tensor(k, dtype=torch.float32)[None]
    best = torch.min(r, 1 / r).min(2)[0].max(1)[0]
    t = best * (best > 1 / thr).float()
    return t.mean(), float(t.double().mean())


def run_reference_kmean(ra, vq, ds, n, gen, seed):
    """kmean_anchors of the reference with scipy's result and the random state behind it recorded"""
    rec = {}
    real = vq.kmeans

    def spy(obs, k, iter=20, **kw):
        st = np.random.get_state()
        rec["index_sets"] = np.array([np.random.choice(obs.shape[0], size=int(k), replace=False) for _ in range(iter)])
        np.random.set_state(st)
        book, dist = real(obs, k, iter=iter, **kw)
        rec.update(obs=np.asarray(obs), book=np.asarray(book), distortion=float(dist), np_state=np.random.get_state(), py_state=random.getstate())
        return book, dist

    vq.kmeans = spy
    try:
        ac.seed_all(seed)
        rec["final"] = ra.kmean_anchors(ds, n=n, img_size=ac.IMG_SIZE, thr=ac.THR, gen=gen, verbose=False)
    finally:
        vq.kmeans = real
    return rec


def replay(ds, n, gen, seed, rec):
    """the reference's loop once more from the recorded random state, with torch's fp32 fitness: k0, v, per-generation fitness, accepted"""
    wh0 = ac.label_wh(ds, ac.IMG_SIZE)
    wh = wh0[(wh0 >= 2.0).any(1)].astype(np.float32)
    fallback = "book" not in rec or len(rec["book"]) != n
    if "book" in rec:
        np.random.set_state(rec["np_state"])
        random.setstate(rec["py_state"])
        k = rec["book"] * wh.std(0)
    else:
        ac.seed_all(seed)
    if fallback:
        k = np.sort(np.random.rand(n * 2)).reshape(n, 2) * ac.IMG_SIZE
    k = ac.by_area(k)
    k0 = k.copy()
    v = ac.draw_mutations(gen, k.shape)
    f, f64 = ref_fitness32(wh, k, ac.THR)
    fit, acc = np.zeros(gen, np.float32), np.zeros(gen, np.int32)
    margin, meangap = np.inf, abs(float(f) - f64) / f64
    for g in range(gen):
        kg = (k.copy() * v[g]).clip(min=2.0)
        fg, fg64 = ref_fitness32(wh, kg, ac.THR)
        fit[g] = float(fg)
        margin = min(margin, abs(float(fg) - float(f)) / float(f))
        meangap = max(meangap, abs(float(fg) - fg64) / fg64)
        if fg > f:
            f, k, acc[g] = fg, kg.copy(), 1
    final = ac.by_area(k).astype(np.float32)
    assert np.array_equal(final, rec["final"]), "the replay from the recorded random state does not reproduce the reference"
    return dict(wh=wh, k0=k0, v=v, fitness=fit, accepted=acc, margin=margin, meangap=meangap, fallback=fallback)


def try_seed(ra, vq, case, seed, dseed=None):
    c = ac.CASES[case]
    ds = ac.make_dataset(case, dseed)
    n, gen = c["n"], c["gen"]
    rec = run_reference_kmean(ra, vq, ds, n, gen, seed)
    rp = replay(ds, n, gen, seed, rec)
    N = len(rp["wh"])
    if case in "ABC" and (N % 64 == 0 or (case == "C" and N <= 4096) or (case != "C" and not 256 < N < 512)):
        return None, f"N = {N}"
    # 1. the restatement's genetic stage
    got = ac.kmean_anchors(ds, n=n, gen=gen, init=rp["k0"], mutations=rp["v"], record=(r1 := {}))
    if not (np.array_equal(got, rec["final"]) and np.array_equal(r1["accepted"], rp["accepted"])):
        return None, "genetic stage differs"
    # 2. decisions away from the summation error
    if not rp["margin"] >= MARGIN_FACTOR * rp["meangap"]:
        return None, f"margin {rp['margin']:.3g} < {MARGIN_FACTOR} x {rp['meangap']:.3g}"
    out = dict(seed=seed, checksum=ac.dataset_checksum(ds), n=n, gen=gen, N=N, k0=torch.from_numpy(rp["k0"]), v=torch.from_numpy(rp["v"]),
               fitness=torch.from_numpy(rp["fitness"]), accepted=torch.from_numpy(rp["accepted"]), final=torch.from_numpy(rec["final"]), fallback=rp["fallback"],
               margin=float(rp["margin"]), meangap=float(rp["meangap"]))
    # 3. k-means away from the rounding edges
    if "book" in rec:
        trace = {}
        book, d, iters = ac.kmeans(rec["obs"], rec["index_sets"], trace)
        if case != "E":
            edge = min(abs(x - ac.KM_THRESH) for x in trace["delta"])
            if edge <= EDGE_MIN or min(trace["gap"]) <= GAP_MIN:
                return None, f"k-means at a rounding edge (stop rule {edge:.3g}, gap {min(trace['gap']):.3g})"
            out.update(kmeans_min_gap=min(trace["gap"]), kmeans_stop_edge=edge)
            if len(book) != len(rec["book"]):
                return None, "codebook sizes differ"
            gap = float(np.abs(book - rec["book"]).max())
            if gap > 2e-6:
                return None, f"restatement vs scipy {gap:.3g}"
            out["kmeans_gap"] = gap
        out.update(index_sets=torch.from_numpy(rec["index_sets"]), book=torch.from_numpy(rec["book"]), distortion=rec["distortion"], kmeans_iters=torch.from_numpy(iters),
                   book_rows=len(rec["book"]))
    # bpr / aat of several anchor sets, the reference's own expressions
    sets = {"k0": rp["k0"], "final": rec["final"].astype(np.float64), "yolov3": np.array(ac.ANCHORS["yolov3"][0], dtype=np.float64).reshape(-1, 2)}
    out["metrics"] = {}
    whr = torch.tensor(rp["wh"])
    for name, k in sets.items():
        r = whr[:, None] / torch.tensor(k, dtype=torch.float32)[None]
        x = torch.min(r, 1 / r).min(2)[0]
        best = x.max(1)[0]
        t = 1 / ac.THR
        out["metrics"][name] = dict(k=torch.from_numpy(np.asarray(k)), **{key: float(val) for key, val in dict(   # fp32 values, held exactly by a float
            bpr=(best > t).float().mean(), aat=(x > t).float().sum(1).mean(), fitness=(best * (best > t).float()).mean(), x_mean=x.mean(), best_mean=best.mean(),
            past_thr_mean=x[x > t].mean()).items()})
    return out, "ok"


def run_check_anchors(ra, ds, family, seed):
    px, strides = ac.ANCHORS[family]
    stride = torch.tensor(strides)
    m = types.SimpleNamespace(anchors=torch.tensor(px, dtype=torch.float32).view(len(px), -1, 2) / stride.view(-1, 1, 1), stride=stride)
    before = m.anchors.clone()
    ac.seed_all(seed)
    ra.check_anchors(ds, types.SimpleNamespace(model=[m]), thr=ac.THR, imgsz=ac.IMG_SIZE)
    assert not torch.equal(before, m.anchors), "check_anchors left the anchors alone (or the shim swallowed an exception)"
    ac.seed_all(seed)
    mine = ac.check_anchors(ds, before.numpy(), strides, record=(rec := {}))
    rel = float((np.abs(mine - m.anchors.numpy()) / np.abs(m.anchors.numpy())).max())
    return dict(before=before, after=m.anchors.clone(), wh=torch.from_numpy(rec["wh"]), bpr=float(rec["bpr"]), new_bpr=float(rec["new_bpr"]), seed=seed), rel


def main():
    ra, vq = reference()
    gold = {"meta": {"scipy": __import__("scipy").__version__, "numpy": np.__version__, "torch": str(torch.__version__)}, "cases": {}, "check": {}}
    for case in ac.CASES:
        for seed in range(32):
            out, why = try_seed(ra, vq, case, seed)
            print(f"case {case} seed {seed}: {why}", flush=True)
            if out is not None:
                gold["cases"][case] = out
                break
        else:
            raise SystemExit(f"case {case}: no seed in 0..31 satisfies the conditions")
    ds = ac.make_dataset("A")
    for family in ac.ANCHORS:
        for seed in range(32):
            out, rel = run_check_anchors(ra, ds, family, seed)
            print(f"check_anchors {family} seed {seed}: restatement vs reference {rel:.3g}", flush=True)
            if rel <= 1e-6:
                out["restatement_gap"] = rel
                gold["check"][family] = out
                break
        else:
            raise SystemExit(f"check_anchors {family}: no seed in 0..31 within 1e-6")
    gold["meta"]["kmeans_gap"] = {c: g.get("kmeans_gap") for c, g in gold["cases"].items()}
    path = ROOT / "tests" / "golden" / "autoanchor.pt"
    torch.save(gold, path)
    torch.load(path, weights_only=True)   # data only: tensors, numbers, strings
    print(path, path.stat().st_size, "bytes", gold["meta"])


if __name__ == "__main__":
    main()
