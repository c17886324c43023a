"""``AutoShape``: the reference's input-robust inference wrapper (models/common.py:766-876) on the MI355X path.

numpy / PIL images of any size go in; each is uploaded once as raw HWC uint8 and letterboxed ON THE DEVICE
(csrc/val_edge.hip: cv2.resize INTER_LINEAR + 114-border + HWC->CHW in one pass, reference utils/augmentations.py:104-134),
the uint8 batch feeds the model's first kernel directly (the /255 of models/common.py:868 happens inside the stem
convolution), then batched NMS and batched scale_boxes (one launch each instead of the per-image loop of :871-872).
``Detections`` has the reference's data attributes, its text half (``str()`` / ``print()`` / ``pandas()``) and ``crop()``, whose boxes come from one launch of
y3_classifier_boxes and one of y3_scale_boxes (csrc/crops.hip, csrc/val_edge.hip) and one copy to the host; show / save / render draw with upstream's Annotator and a
font, neither of which is here, and are not provided.
"""
from __future__ import annotations

import time
from pathlib import Path

import numpy as np
import torch
from torch import nn

from . import ops
from .general import non_max_suppression_batched, scale_boxes_batched
from .yolo import make_divisible


def letterbox_geometry(shape, new_shape=(640, 640), auto=False, scaleup=True, stride=32):
    """(new_h, new_w, top, left, ratio, (dw, dh)) exactly as reference utils/augmentations.py:104-134 computes them
    (Python round() = round-half-even, like the reference)."""
    if isinstance(new_shape, int):
        new_shape = (new_shape, new_shape)
    r = min(new_shape[0] / shape[0], new_shape[1] / shape[1])
    if not scaleup:
        r = min(r, 1.0)
    new_unpad = round(shape[1] * r), round(shape[0] * r)
    dw, dh = new_shape[1] - new_unpad[0], new_shape[0] - new_unpad[1]
    if auto:
        dw, dh = dw % stride, dh % stride
    dw /= 2
    dh /= 2
    top, bottom = round(dh - 0.1), round(dh + 0.1)
    left, right = round(dw - 0.1), round(dw + 0.1)
    return new_unpad[1], new_unpad[0], top, left, (r, r), (dw, dh), (new_unpad[1] + top + bottom, new_unpad[0] + left + right)


def letterbox_batch(ims, shape1, device, color=114):
    """list of HWC uint8 numpy images -> (n, 3, H1, W1) uint8 device batch, letterboxed to exactly `shape1` (auto=False)."""
    x = torch.empty(len(ims), 3, shape1[0], shape1[1], dtype=torch.uint8, device=device)
    for i, im in enumerate(ims):
        nh, nw, top, left, _, _, full = letterbox_geometry(im.shape[:2], shape1)
        if tuple(full) != tuple(shape1):
            raise ValueError(f"letterbox of {im.shape[:2]} to {shape1} gives {full}")
        src = torch.from_numpy(np.ascontiguousarray(im)).to(device, non_blocking=True)
        ops.letterbox_u8(src, x, i, nh, nw, top, left, color)
    return x


class Detections:
    """Result container with the reference's data attributes (models/common.py:879-903)."""

    def __init__(self, ims, pred, files, times=(0.0, 0.0, 0.0), names=None, shape=None):
        d = pred[0].device if pred else torch.device("cpu")
        gn = [torch.tensor([*(im.shape[i] for i in [1, 0, 1, 0]), 1, 1], device=d) for im in ims]
        self.ims, self.pred, self.names, self.files, self.times = ims, pred, names, files, times
        self.xyxy = pred
        self.xywh = [torch.cat((_xyxy2xywh(x[:, :4]), x[:, 4:]), 1) for x in pred]
        self.xyxyn = [x / g for x, g in zip(self.xyxy, gn)]
        self.xywhn = [x / g for x, g in zip(self.xywh, gn)]
        self.n = len(self.pred)
        self.t = tuple(t * 1e3 / max(self.n, 1) for t in times)
        self.s = tuple(shape) if shape is not None else None

    def __len__(self):
        return self.n

    def tolist(self):
        return [Detections([self.ims[i]], [self.pred[i]], [self.files[i]], self.times, self.names, self.s) for i in range(self.n)]

    def _name(self, c):
        return self.names[c] if self.names is not None else str(c)

    def __str__(self):
        """reference models/common.py:906-913, 950-952 (`_run(pprint=True)`): per image its size and "2 persons, 1 tie", then the speed line.  The class counts of device
        predictions come from the histogram of one export launch and one copy (outputs.class_histograms), not from a `unique()` and a sum per class and image."""
        from .outputs import class_histograms

        nc = len(self.names) if self.names is not None else 1000   # (DetectMultiBackend's default names cover 1000 classes)
        s = ""
        for i, (im, hist) in enumerate(zip(self.ims, class_histograms(self.pred, nc))):
            s += f"\nimage {i + 1}/{len(self.pred)}: {im.shape[0]}x{im.shape[1]} "
            if self.pred[i].shape[0]:
                for c, n in hist.items():
                    s += f"{n} {self._name(c)}{'s' * (n > 1)}, "
                s = s.rstrip(", ")
            else:
                s += "(no detections)"
        s = s.lstrip("\n")
        return f"{s}\nSpeed: %.1fms pre-process, %.1fms inference, %.1fms NMS per image at shape {self.s}" % self.t

    def __repr__(self):
        return f"YOLOv3 {self.__class__} instance\n" + self.__str__()

    def print(self):
        import logging

        logging.getLogger("yolov3_amd").info(self.__str__())

    def pandas(self):
        """reference models/common.py:990-998: a copy whose xyxy / xyxyn / xywh / xywhn are pandas DataFrames (pandas is imported here, not with the package)"""
        import pandas as pd
        from copy import copy

        new = copy(self)
        ca = "xmin", "ymin", "xmax", "ymax", "confidence", "class", "name"
        cb = "xcenter", "ycenter", "width", "height", "confidence", "class", "name"
        for k, c in zip(["xyxy", "xyxyn", "xywh", "xywhn"], [ca, ca, cb, cb]):
            a = [[[*x[:5], int(x[5]), self._name(int(x[5]))] for x in t.tolist()] for t in getattr(self, k)]
            setattr(new, k, [pd.DataFrame(x, columns=c) for x in a])
        return new

    def crop(self, save=True, save_dir="runs/detect/exp", exist_ok=False):
        """reference models/common.py:974-980 (`_run(crop=True)`, :916-928): per image, in reversed(pred) order, {"box", "conf", "cls", "label", "im"} with `im` the crop
        of upstream save_one_box (gain 1.02, pad 10, not squared, clipped to the image; ims[i][y1:y2, x1:x2, ::-1]).  The boxes of all images are formed on the device
        (crop_boxes) and read back in one copy.  save=True writes every crop to save_dir/crops/<class name>/<file> as save_one_box does (Pillow, quality=95,
        subsampling=0, an existing name incremented); the un-annotated whole images the reference's `save` also writes next to them are not written."""
        save_dir = increment_path(save_dir, exist_ok, mkdir=True) if save else None
        live = [i for i, p in enumerate(self.pred) if p.shape[0]]
        boxes = crop_boxes([self.pred[i] for i in live], [self.ims[i].shape[:2] for i in live]) if live else []
        crops = []
        for i, b in zip(live, boxes):
            im, pred = self.ims[i], self.pred[i]
            for j in reversed(range(pred.shape[0])):
                *box, conf, cls = pred[j]
                name = self._name(int(cls))
                x1, y1, x2, y2 = b[j]
                cut = im[y1:y2, x1:x2, ::-1]
                if save:
                    file = increment_path(save_dir / "crops" / name / self.files[i]).with_suffix(".jpg")
                    file.parent.mkdir(parents=True, exist_ok=True)
                    from PIL import Image

                    Image.fromarray(np.ascontiguousarray(cut[..., ::-1])).save(str(file), quality=95, subsampling=0)
                crops.append({"box": box, "conf": conf, "cls": cls, "label": f"{name} {conf:.2f}", "im": cut})
        return crops


def increment_path(path, exist_ok=False, sep="", mkdir=False):
    """upstream increment_path with the reference's sep="" (utils/general.py:862): runs/exp -> runs/exp2, runs/exp3, ...; a file keeps its suffix"""
    path = Path(path)
    if path.exists() and not exist_ok:
        path, suffix = (path.with_suffix(""), path.suffix) if path.is_file() else (path, "")
        n = 2
        while Path(f"{path}{sep}{n}{suffix}").exists():
            n += 1
        path = Path(f"{path}{sep}{n}{suffix}")
    if mkdir:
        path.mkdir(parents=True, exist_ok=True)
    return path


def crop_boxes(pred, shapes, gain=1.02, pad=10, square=False):
    """The integer boxes of upstream save_one_box for a list of (n, 6) DEVICE predictions in native pixels and the (h, w) of their images -> per image an (n, 4) int
    list [x1, y1, x2, y2]: y3_classifier_boxes, then y3_scale_boxes with gain 1 and pad 0 (its clip to the image), then ONE copy to the host."""
    counts = [int(p.shape[0]) for p in pred]
    for p in pred:
        ops.require_gpu(p, "Detections.crop")
    dev = pred[0].device
    rows = torch.zeros(len(pred), max(counts), 6, dtype=torch.float32, device=dev)
    for i, p in enumerate(pred):
        rows[i, : counts[i]] = p
    counts_t = torch.tensor(counts, dtype=torch.int32).to(dev, non_blocking=True)
    boxes = ops.classifier_boxes(rows, counts_t, gain, pad, square)
    params = torch.tensor([[1.0, 0.0, 0.0, float(w), float(h)] for h, w in shapes], dtype=torch.float32).to(dev, non_blocking=True)
    ops.scale_boxes_raw(boxes, boxes.stride(0), 4, counts_t, len(pred), boxes.shape[1], params)
    host = boxes.to(torch.int32).tolist()
    return [host[i][: counts[i]] for i in range(len(pred))]


def _xyxy2xywh(x):
    y = x.clone()
    y[..., 0] = (x[..., 0] + x[..., 2]) / 2
    y[..., 1] = (x[..., 1] + x[..., 3]) / 2
    y[..., 2] = x[..., 2] - x[..., 0]
    y[..., 3] = x[..., 3] - x[..., 1]
    return y


class AutoShape(nn.Module):
    conf = 0.25  # NMS confidence threshold
    iou = 0.45  # NMS IoU threshold
    agnostic = False
    multi_label = False
    classes = None
    max_det = 1000
    amp = False

    def __init__(self, model, verbose=True):
        super().__init__()
        for k in ("yaml", "nc", "hyp", "names", "stride", "abc"):
            if hasattr(model, k):
                setattr(self, k, getattr(model, k))
        self.dmb = type(model).__name__ == "DetectMultiBackend"
        self.pt = True
        self.model = model.eval()
        det = self.model.model.model[-1] if self.dmb else self.model.model[-1]
        det.inplace = False
        det.export = True  # no raw head tensors: the decode kernel then skips writing them

    @torch.no_grad()
    def forward(self, ims, size=640, augment=False, profile=False):
        t0 = time.perf_counter()
        if isinstance(size, int):
            size = (size, size)
        p = next(self.model.parameters())
        if isinstance(ims, torch.Tensor):
            return self.model(ims.to(p.device).type_as(p), augment=augment)
        n, ims = (len(ims), list(ims)) if isinstance(ims, (list, tuple)) else (1, [ims])
        shape0, shape1, files = [], [], []
        for i, im in enumerate(ims):
            f = f"image{i}"
            if isinstance(im, (str, Path)):
                if str(im).startswith("http"):
                    raise ValueError("AutoShape: URLs are not fetched here (no network I/O on the hot path); pass a decoded image")
                from PIL import Image

                im, f = np.asarray(Image.open(im)), im
            elif not isinstance(im, np.ndarray):  # PIL.Image
                im, f = np.asarray(im), getattr(im, "filename", f) or f
            files.append(Path(f).with_suffix(".jpg").name)
            if im.shape[0] < 5:  # CHW
                im = im.transpose((1, 2, 0))
            im = im[..., :3] if im.ndim == 3 else np.stack((im,) * 3, -1)  # enforce 3 channels (cv2.COLOR_GRAY2BGR replicates)
            s = im.shape[:2]
            shape0.append(s)
            g = max(size) / max(s)
            shape1.append([int(y * g) for y in s])
            ims[i] = np.ascontiguousarray(im)
        stride = int(self.stride.max()) if isinstance(self.stride, torch.Tensor) else int(self.stride)
        shape1 = [make_divisible(x, stride) for x in np.array(shape1).max(0)]
        x = letterbox_batch(ims, shape1, p.device)  # uint8; the model's first kernel divides by 255
        t1 = time.perf_counter()
        net = self.model.model if self.dmb else self.model   # the DetectionModel itself: it takes the uint8 batch (a DetectMultiBackend would cast it to half without the /255)
        y = net(x, augment=augment)
        t2 = time.perf_counter()
        rows, counts_t, counts = non_max_suppression_batched(y[0], self.conf, self.iou, self.classes, self.agnostic, self.multi_label, max_det=self.max_det)
        scale_boxes_batched(shape1, rows, counts_t, shape0)
        pred = [rows[i, :c] for i, c in enumerate(counts)]
        t3 = time.perf_counter()
        return Detections(ims, pred, files, (t1 - t0, t2 - t1, t3 - t2), getattr(self, "names", None), x.shape)
