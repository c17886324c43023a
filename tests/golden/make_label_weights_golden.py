"""Generate tests/golden/label_weights.pt from the UNMODIFIED reference (utils.general.labels_to_class_weights / labels_to_image_weights through oracle/ref_shim.py)
and Python's random.choices.

    python tests/golden/make_label_weights_golden.py

Only where the reference tree is present.  The file holds data only.  Per case (tests/label_weights_cases.py) it records the checksum of the rebuilt labels, the
reference's class weights, `maps` and the class weights of the epoch prologue cw = (class_weights * nc).numpy() * (1 - maps) ** 2 / nc (train.py:333,360), the
reference's image weights for cw, and -- except for E, whose total is zero -- a seed, the indices random.choices(range(n), weights=iw, k=n) returns after
random.seed(seed), the value random.random() returns next and the measured margin.

The seed is the first in 0..31 for which every draw u * total lies at least 1e-9 * total away from every cumulative boundary of the reference's iw (for A over
3 n draws, whose indices are recorded too: the first n of them are the k = n draws).  A parallel fp64 scan over non-negative terms moves a boundary by at most
about n 2^-53 relative (2e-12 at n = 20 000), so the device's indices must then be the reference's.
"""
import random
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import label_weights_cases as lc  # noqa: E402
from oracle import ref_shim  # noqa: E402


def reference():
    ref_shim.install()
    from utils.general import labels_to_class_weights, labels_to_image_weights  # type: ignore

    return labels_to_class_weights, labels_to_image_weights


def run_case(ref_cw, ref_iw, case):
    """everything the golden holds for one case, from the reference"""
    labels, nc, maps = lc.make_labels(case), lc.CASES[case]["nc"], lc.make_maps(case)
    n = len(labels)
    class_weights = ref_cw(labels, nc)
    cw = (class_weights * nc).numpy() * (1 - maps) ** 2 / nc
    iw = ref_iw(labels, nc=nc, class_weights=cw)
    assert class_weights.dtype == torch.float32 and iw.dtype == np.float64 and iw.shape == (n,)
    out = dict(checksum=lc.checksum(labels), n=n, N=int(sum(len(l) for l in labels)), nc=nc, class_weights=class_weights, maps=torch.from_numpy(maps), cw=torch.from_numpy(cw),
               iw=torch.from_numpy(iw), iw_ones=torch.from_numpy(ref_iw(labels, nc=nc, class_weights=np.ones(nc))), seed=-1)
    if not iw.sum() > 0:
        return out
    draws = 3 * n if case == "A" else n
    for seed in range(32):
        random.seed(seed)
        margin = lc.boundary_margin(iw, [random.random() for _ in range(draws)])
        print(f"case {case} seed {seed}: margin {margin:.3g}", flush=True)
        if margin >= lc.MARGIN:
            break
    else:
        raise SystemExit(f"case {case}: no seed in 0..31 keeps every draw {lc.MARGIN} away from the boundaries")
    random.seed(seed)
    indices = random.choices(range(n), weights=iw, k=n)
    out.update(seed=seed, margin=margin, indices=torch.tensor(indices, dtype=torch.int32), next_random=random.random())
    if case == "A":
        random.seed(seed)
        out["indices_3n"] = torch.tensor(random.choices(range(n), weights=iw, k=3 * n), dtype=torch.int32)
        out["next_random_3n"] = random.random()
    return out


def main():
    ref_cw, ref_iw = reference()
    gold = {"meta": {"numpy": np.__version__, "torch": str(torch.__version__), "python": sys.version.split()[0]}, "cases": {c: run_case(ref_cw, ref_iw, c) for c in lc.CASES}}
    assert ref_cw([None], 80).numel() == 0
    path = ROOT / "tests" / "golden" / "label_weights.pt"
    torch.save(gold, path)
    torch.load(path, weights_only=True)   # data only: tensors, numbers, strings
    print(path, path.stat().st_size, "bytes", gold["meta"])


if __name__ == "__main__":
    main()
