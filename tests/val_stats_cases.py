"""Seeded inputs of the device-side validation statistics (yolov3_amd.metrics.ValStats / ConfusionMatrix): shared by the fixture generator
tests/golden/make_val_stats_golden.py (which runs the unmodified reference on them) and by tests/test_val_stats_*.py (which regenerate them and compare).
Test infrastructure: CPU generators only, nothing here is imported by the product."""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

from oracle import yolo_oracle as yo  # noqa: E402

# name -> keyword arguments of oracle.yolo_oracle.synth_ap_stats (classes with labels and no predictions, and the reverse, included)
AP_SYNTH_CASES = {
    "mixed": dict(seed=3),
    "single_iou": dict(seed=4, n_iou=1),
    "few": dict(seed=5, n_det=7, n_lab=5, nc=3, absent=0),
    "one_class": dict(seed=6, n_det=120, n_lab=40, nc=2, absent=0),
    "wide": dict(seed=8, n_det=2500, n_lab=900, nc=12, absent=2),
}
AP_CASES = [*AP_SYNTH_CASES, "large"]


def large_ap_case(seed=21, n=20000, n_lab=6000, nc=80, n_iou=10):
    """about 20 000 detections over 80 classes.  20 000 fp32 `torch.rand` draws tie (about a dozen pairs), which the reference's unstable argsort leaves
    undefined: the confidences are a seeded permutation of (k + 0.5) / n instead, pairwise distinct in fp32."""
    g = torch.Generator().manual_seed(seed)
    conf = ((torch.randperm(n, generator=g).double() + 0.5) / n).float()
    q = torch.rand(n, generator=g) * (0.3 + 0.7 * conf)
    tp = q[:, None] > torch.linspace(0.45, 0.9, n_iou)[None, :]
    pred_cls = torch.randint(0, nc - 3, (n,), generator=g).float()       # the last three classes have labels and no predictions
    target_cls = torch.randint(2, nc, (n_lab,), generator=g).float()     # classes 0 and 1 have predictions only
    return tp.numpy(), conf.numpy(), pred_cls.numpy(), target_cls.numpy()


def ap_case(name):
    """(tp (n, T) bool, conf (n,) fp32, pred_cls (n,), target_cls (n_labels,)) NumPy, as val.py:424 hands them to ap_per_class"""
    return large_ap_case() if name == "large" else yo.synth_ap_stats(**AP_SYNTH_CASES[name])


def tied_ap_case(seed=31, n=6000, n_lab=1500, nc=9, n_iou=10):
    """confidences quantised to fp16 steps of a narrow range: many exact duplicates within every class"""
    g = torch.Generator().manual_seed(seed)
    conf = (0.2 + 0.1 * torch.rand(n, generator=g)).half().float()
    q = torch.rand(n, generator=g) * (0.3 + 0.7 * conf * 3)
    tp = q[:, None] > torch.linspace(0.45, 0.9, n_iou)[None, :]
    return tp.numpy(), conf.numpy(), torch.randint(0, nc, (n,), generator=g).float().numpy(), torch.randint(0, nc, (n_lab,), generator=g).float().numpy()


def coco_scale_case(seed=41, n=1_500_000, n_lab=36_000, nc=80, n_iou=10):
    """COCO-val scale: 5000 images x 300 detections, 80 classes with a dominant class 0 (about a quarter of the rows); every class's hits stay below its labels"""
    g = torch.Generator().manual_seed(seed)
    conf = torch.rand(n, generator=g)
    pred_cls = torch.where(torch.rand(n, generator=g) < 0.25, torch.zeros(n), torch.randint(0, nc, (n,), generator=g).float())
    q = torch.rand(n, generator=g) * conf
    tp = q[:, None] > torch.linspace(0.9, 0.99, n_iou)[None, :]
    target_cls = torch.where(torch.rand(n_lab, generator=g) < 0.25, torch.zeros(n_lab), torch.randint(0, nc, (n_lab,), generator=g).float())
    return tp.numpy(), conf.numpy(), pred_cls.numpy(), target_cls.numpy()


CONFUSION = dict(nc=5, conf=0.25, iou_thres=0.45, seed=17, images=14)


def box_iou_np(a, b):
    """upstream box_iou (N, 4) x (M, 4) in fp32, through torch like the reference"""
    a, b = torch.as_tensor(a), torch.as_tensor(b)
    a1, a2 = a.float().unsqueeze(1).chunk(2, 2)
    b1, b2 = b.float().unsqueeze(0).chunk(2, 2)
    inter = (torch.min(a2, b2) - torch.max(a1, b1)).clamp_(0).prod(2)
    return inter / ((a2 - a1).prod(2) + (b2 - b1).prod(2) - inter + 1e-7)


def confusion_images(seed=CONFUSION["seed"], images=CONFUSION["images"], nc=CONFUSION["nc"]):
    """a seeded sequence of images [(detections (n, 6) fp32 [x1, y1, x2, y2, conf, cls], labels (m, 5) fp32 [cls, x1, y1, x2, y2])]: jittered copies of the labels
    (sometimes with another class, sometimes two on one label), stray boxes, confidences on both sides of the threshold; image 2 has no detections,
    image 4 no labels, image 6 no pair above the IoU threshold, image 8 only detections below the confidence threshold, image 10 neither"""
    g = torch.Generator().manual_seed(seed)
    out = []
    for i in range(images):
        m = int(torch.randint(2, 7, (1,), generator=g))
        xy = torch.rand(m, 2, generator=g) * 400
        wh = 40 + torch.rand(m, 2, generator=g) * 160
        lab = torch.cat((torch.randint(0, nc, (m, 1), generator=g).float(), xy, xy + wh), 1)
        rows = []
        for l in range(m):
            for _ in range(int(torch.randint(0, 3, (1,), generator=g))):
                jit = (torch.rand(4, generator=g) - 0.5) * 0.35 * torch.cat((wh[l], wh[l]))
                cls = lab[l, 0] if float(torch.rand(1, generator=g)) < 0.7 else torch.randint(0, nc, (1,), generator=g).float()[0]
                rows.append(torch.cat((lab[l, 1:] + jit, 0.05 + 0.95 * torch.rand(1, generator=g), cls[None])))
        for _ in range(int(torch.randint(0, 4, (1,), generator=g))):
            p = torch.rand(2, generator=g) * 500
            rows.append(torch.cat((p, p + 30 + torch.rand(2, generator=g) * 200, 0.05 + 0.95 * torch.rand(1, generator=g), torch.randint(0, nc, (1,), generator=g).float())))
        det = torch.stack(rows) if rows else torch.zeros(0, 6)
        if i == 2:
            det = torch.zeros(0, 6)
        if i == 4:
            lab = torch.zeros(0, 5)
        if i == 6 and det.shape[0]:
            det[:, :4] += 2000.0
        if i == 8 and det.shape[0]:
            det[:, 4] *= 0.2
        if i == 10:
            det, lab = torch.zeros(0, 6), torch.zeros(0, 5)
        out.append((det.contiguous(), lab.contiguous()))
    return out
