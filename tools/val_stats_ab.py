"""A/B of the last step of a validation run at COCO-val scale (1.5 M rows, 80 classes, T = 10; tests/val_stats_cases.py::coco_scale_case):
  (a) the host path: device->host copy of the statistics + yolov3_amd.metrics.ap_per_class (NumPy),
  (b) the device path: yolov3_amd.metrics.ValStats.compute() including its read-back (csrc/val_stats.hip),
interleaved, five rounds each after a warm-up, plus the kernel-by-kernel split of one (b).  Run on the GPU machine under one time limit:

    timeout -k 10 600 python tools/val_stats_ab.py --out profiles/val_stats_ab.txt
"""
from __future__ import annotations

import argparse
import platform
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))


def cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return platform.processor() or "unknown"


def main():
    import val_stats_cases as vc
    from yolov3_amd import metrics

    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    tp, conf, pc, tc = vc.coco_scale_case()
    d_tp, d_conf, d_pc, d_tc = (torch.from_numpy(x).to(dev) for x in (tp, conf, pc, tc))
    st = metrics.ValStats(80, 10, dev)
    st.append_rows(d_tp, d_conf, d_pc)
    st.add_labels(d_tc)
    torch.cuda.synchronize()

    def host_path():
        t0 = time.perf_counter()
        cols = [x.cpu().numpy() for x in (d_tp, d_conf, d_pc, d_tc)]
        t1 = time.perf_counter()
        res = metrics.ap_per_class(*cols)
        return time.perf_counter() - t0, t1 - t0, res

    def device_path():
        st._result = None
        t0 = time.perf_counter()
        res = st.compute()
        return time.perf_counter() - t0, res

    host_path(), device_path()   # warm-up
    ta, tcopy, tb = [], [], []
    for _ in range(a.rounds):
        x = host_path()
        ta.append(x[0]); tcopy.append(x[1])
        y = device_path()
        tb.append(y[0])
    diff = max(float(np.abs(p - q).max(initial=0.0)) for p, q in zip(x[2], y[1]))
    lines = [f"val_stats_ab: {tp.shape[0]} rows, 80 classes, T = {tp.shape[1]}, {a.rounds} interleaved rounds after one warm-up",
             f"device: {torch.cuda.get_device_name(0)}   host CPU: {cpu_model()}",
             "(a) host path  (copy of the statistics + metrics.ap_per_class): " + "  ".join(f"{t * 1e3:9.2f}" for t in ta) + f"   median {statistics.median(ta) * 1e3:.2f} ms"
             f"  (the copy alone: median {statistics.median(tcopy) * 1e3:.2f} ms)",
             "(b) device path (ValStats.compute() incl. read-back):            " + "  ".join(f"{t * 1e3:9.2f}" for t in tb) + f"   median {statistics.median(tb) * 1e3:.2f} ms",
             f"(b) below (a) in every round: {all(q < p for p, q in zip(ta, tb))}   max |a - b| over the 7 outputs: {diff:.3e} (fp32 scores of this size tie: (a) ranks ties as the unstable argsort leaves them, (b) by arrival)"]
    try:
        from torch.profiler import ProfilerActivity, profile

        st._result = None
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            st.compute()
            torch.cuda.synchronize()
        lines.append("kernels of one (b):")
        for e in sorted(prof.key_averages(), key=lambda e: -e.device_time_total):
            if e.device_time_total > 0:
                lines.append(f"  {e.device_time_total / 1e3:9.3f} ms  x{e.count:<3d} {e.key[:110]}")
    except Exception as ex:   # the split is a report, the medians above are the measurement
        lines.append(f"kernel split unavailable: {type(ex).__name__}: {ex}")
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text)


if __name__ == "__main__":
    main()
