"""Fixtures of the model-ensemble tests, from the UNMODIFIED reference (through oracle/ref_shim.py).  Run in the build container only:

    python tests/golden/make_ensemble_golden.py

* ``ref_tiny_w025_b_fp16.pt``: a second checkpoint pickled by the reference the way train.py:470-488 saves one -- the recipe of make_golden.py::gen_ckpt_fixture with
  other seeds.  Its width multiple is 0.1875 instead of 0.25 (0.32 M parameters): a half-precision pickle of the 0.25 model is 1.2 MB, above the repository's
  limit of 1 MiB for a committed file.  The row counts of the two members are the same either way (they depend on the strides alone).
* ``ensemble.pt``: the reference's ``attempt_load([a, b])`` (models/experimental.py:88-136) -- its ``names`` / ``nc`` / ``stride`` and its decoded prediction on the
  batch of ref_tiny_w025_eval.pt (seed 9; checksum stored).

Two things around the reference call are the caller's and not the reference's:
* ``torch_load`` is ultralytics' patch of ``torch.load`` (un-vendored): it passes ``weights_only=False``, which is all that is restated here;
* ``attempt_load`` reads ``model[0].nc``, which train.py attaches to the model before it saves it (``model.nc = nc``) and gen_ckpt_fixture's recipe did not: the loader
  below attaches the Detect head's count to a model that lacks it, for the existing checkpoint as for the new one.
"""
from __future__ import annotations

import sys
from copy import deepcopy
from pathlib import Path

import torch
import yaml

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))

from oracle import ref_shim  # noqa: E402

OUT = Path(__file__).resolve().parent
CFG = ROOT / "yolov3_amd" / "cfg"
A, B = OUT / "ref_tiny_w025_fp16.pt", OUT / "ref_tiny_w025_b_fp16.pt"


def checksum(t: torch.Tensor) -> float:
    return float(t.double().abs().sum())


def gen_second_ckpt(ns):
    d = yaml.safe_load(open(CFG / "yolov3-tiny.yaml"))
    d["width_multiple"] = 0.1875
    torch.manual_seed(17)
    m = ns.DetectionModel(d, ch=3, nc=80)
    g = torch.Generator().manual_seed(18)
    for mod in m.modules():
        if isinstance(mod, torch.nn.BatchNorm2d):
            mod.weight.data = torch.rand(mod.weight.shape, generator=g) + 0.5
            mod.bias.data = torch.randn(mod.bias.shape, generator=g) * 0.1
            mod.running_mean = torch.randn(mod.running_mean.shape, generator=g) * 0.1
            mod.running_var = torch.rand(mod.running_var.shape, generator=g) + 0.5
    m.names = {i: f"b{i}" for i in range(80)}
    ckpt = {"epoch": 7, "best_fitness": None, "model": deepcopy(m).half(), "ema": None, "updates": None, "optimizer": None, "opt": {}, "git": None, "date": "2026-10-19"}
    torch.save(ckpt, B)
    print("ckpt b", B.stat().st_size, sum(p.numel() for p in m.parameters()))
    assert B.stat().st_size < (1 << 20)


def gen_ensemble(ns):
    import models.experimental as exp  # type: ignore

    def torch_load(f, **kw):
        ckpt = torch.load(f, weights_only=False, **kw)
        for k in ("ema", "model"):
            mod = ckpt.get(k)
            if mod is not None and not hasattr(mod, "nc"):
                mod.nc = mod.model[-1].nc   # train.py: `model.nc = nc` ahead of the save
        return ckpt

    exp.torch_load = torch_load
    assert A.exists() and B.exists()   # (attempt_download leaves an existing file alone)
    ens = exp.attempt_load([str(A), str(B)], device=torch.device("cpu"))
    assert type(ens).__name__ == "Ensemble" and len(ens) == 2
    x = torch.rand(2, 3, 96, 160, generator=torch.Generator().manual_seed(9))
    with torch.no_grad():
        y, none = ens(x)
        parts = [m(x)[0] for m in ens]
    assert none is None and torch.equal(y, torch.cat(parts, 1))
    torch.save({"x_sum": checksum(x), "pred": y.clone(), "rows": [int(p.shape[1]) for p in parts], "names": dict(ens.names), "nc": int(ens.nc),
                "stride": [float(s) for s in ens.stride]}, OUT / "ensemble.pt")
    print("ensemble", tuple(y.shape), [int(p.shape[1]) for p in parts], ens.nc, ens.stride.tolist(), (OUT / "ensemble.pt").stat().st_size)


if __name__ == "__main__":
    ns = ref_shim.load()
    torch.manual_seed(0)
    gen_second_ckpt(ns)
    gen_ensemble(ns)
