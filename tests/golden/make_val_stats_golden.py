"""Generate tests/golden/val_stats.pt by running the UNMODIFIED reference (through oracle/ref_shim.py) on the seeded inputs of tests/val_stats_cases.py:
`ap_per_class` of utils/metrics.py on every AP case and `ConfusionMatrix.matrix` after the image sequence, called as val.py:386-406 calls it.
Run where the reference tree is present:

    python tests/golden/make_val_stats_golden.py

The fixture stores reference OUTPUTS and input checksums only; the tests regenerate the inputs from their seeds."""
from __future__ import annotations

import importlib
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import val_stats_cases as vc  # noqa: E402
from oracle import ref_shim  # noqa: E402

OUT = Path(__file__).resolve().parent


def main():
    ref_shim.load()
    rm = importlib.import_module("utils.metrics")
    out = {"ap": {}, "confusion": {}}
    for name in vc.AP_CASES:
        tp, conf, pc, tc = vc.ap_case(name)
        assert len(np.unique(conf)) == conf.shape[0], f"{name}: score ties make the reference's argsort ambiguous"
        res = rm.ap_per_class(tp, conf, pc, tc, plot=False, names={})
        out["ap"][name] = {"in_sum": float(tp.sum() + conf.astype(np.float64).sum() + pc.sum() + tc.sum()), "shape": tuple(tp.shape),
                           "out": [torch.as_tensor(np.asarray(r).copy()) for r in res]}
        print("ap", name, tp.shape, "classes", len(res[6]), "mAP50", float(res[5][:, 0].mean()), "mAP", float(res[5].mean()))
    c = vc.CONFUSION
    cm = rm.ConfusionMatrix(nc=c["nc"], conf=c["conf"], iou_thres=c["iou_thres"])
    in_sum, kinds = 0.0, {"no_det": 0, "no_lab": 0, "no_match": 0, "below_conf": 0}
    for det, lab in vc.confusion_images():
        in_sum += float(det.double().abs().sum() + lab.double().abs().sum())
        if det.shape[0] and lab.shape[0]:
            iou = vc.box_iou_np(lab[:, 1:], det[det[:, 4] > c["conf"]][:, :4])
            above = iou[iou > c["iou_thres"]]
            assert len(torch.unique(above)) == above.numel(), "equal IoUs above the threshold: the reference's argsort is ambiguous"
            kinds["no_match"] += above.numel() == 0
            kinds["below_conf"] += int((det[:, 4] <= c["conf"]).any())
        kinds["no_det"] += det.shape[0] == 0 and lab.shape[0] > 0
        kinds["no_lab"] += lab.shape[0] == 0
        if det.shape[0] == 0:              # val.py:386-391
            if lab.shape[0]:
                cm.process_batch(detections=None, labels=lab[:, 0])
            continue
        if lab.shape[0]:                   # val.py:400-406
            cm.process_batch(det.clone(), lab.clone())
    assert all(v > 0 for v in kinds.values()), kinds
    out["confusion"] = {"in_sum": in_sum, "matrix": torch.as_tensor(cm.matrix.copy()), **c}
    print("confusion", kinds, "\n", cm.matrix)
    torch.save(out, OUT / "val_stats.pt")
    print("val_stats.pt", (OUT / "val_stats.pt").stat().st_size, "bytes")


if __name__ == "__main__":
    main()
