"""Host-side mirror of the metric-matching step of reference val.py: ``process_batch`` (:147-188) with the reference
signature, and a batched form that consumes the batched NMS output without a per-image Python loop or device->host
copies.  The matching runs in csrc/val_edge.hip.  ``run_batches`` is the loop of val.py:351-428 itself: forward, batched
NMS, box / label scaling, matching and the statistics of the run (``metrics.ValStats``, ``metrics.ConfusionMatrix``: csrc/val_stats.hip) all stay on the
device; per batch the host reads the NMS counts and nothing else, and one small block at the end."""
from __future__ import annotations

import torch

from . import ops


def process_batch(detections, labels, iouv):
    """Drop-in for reference val.py:147: detections (N, 6) [x1,y1,x2,y2,conf,cls], labels (M, 5) [cls,x1,y1,x2,y2], iouv (T,)
    -> bool (N, T) on ``iouv.device``.  Exact IoU ties between two labels of one detection resolve to the larger label index
    (what numpy's reversed argsort gives the reference for <= 16 candidate pairs; undefined there beyond that)."""
    ops.require_gpu(detections, "process_batch")
    dev = detections.device
    n = detections.shape[0]
    if n == 0:
        return torch.zeros(0, iouv.numel(), dtype=torch.bool, device=iouv.device)
    if n > 4096:
        raise ValueError("process_batch: more than 4096 detections per image is not supported")
    dets = detections if (detections.dtype == torch.float32 and detections.stride(1) == 1) else detections.float().contiguous()
    lab = labels.to(dev, torch.float32).contiguous()
    offs = torch.tensor([0, lab.shape[0]], dtype=torch.int32).to(dev, non_blocking=True)
    thr = iouv.to(dev, torch.float32).contiguous()
    correct = ops.match_detections_raw(dets, n * dets.stride(0), dets.stride(0), None, 1, n, lab, offs, thr)
    return correct[0].bool().to(iouv.device)


def process_batch_batched(rows, counts, labels, label_offsets, iouv):
    """Matching for a whole batch in one launch: rows (bs, max_det, 6) fp32 + counts (device int32, or None) as returned by
    `non_max_suppression_batched` (after `scale_boxes_batched`), labels (nl, 5) fp32 [cls,x1,y1,x2,y2] grouped by image with
    label_offsets (bs+1 int32: image i owns labels[label_offsets[i]:label_offsets[i+1]]).  Returns uint8 (bs, max_det, T) on
    the device, rows beyond counts[i] are 0."""
    ops.require_gpu(rows, "process_batch_batched")
    if rows.dtype != torch.float32 or rows.dim() != 3 or not rows.is_contiguous():
        raise TypeError("process_batch_batched expects the contiguous (bs, max_det, 6) fp32 NMS output")
    dev = rows.device
    lab = labels.to(dev, torch.float32).contiguous()
    offs = label_offsets.to(dev, torch.int32).contiguous()
    if offs.numel() != rows.shape[0] + 1:
        raise ValueError("label_offsets must hold bs + 1 entries")
    thr = iouv.to(dev, torch.float32).contiguous()
    return ops.match_detections_raw(rows, rows.stride(0), rows.stride(1), counts, rows.shape[0], rows.shape[1], lab, offs, thr)


class _infer_dtype:
    """``with _infer_dtype(model, half, dtype):`` -- the model's inference plans run in `dtype` (half: float16) inside the block, whatever its parameters are: fp32
    masters are read as they are and rounded once when the filter banks are packed (no ``model.half()`` ... ``model.float()`` round trip, reference val.py).
    Neither given: the block changes nothing."""

    def __init__(self, model, half=False, dtype=None):
        self.dtype = dtype if dtype is not None else (torch.float16 if half else None)
        self.target = None
        if self.dtype is not None:
            self.target = model if hasattr(model, "infer_dtype") else getattr(model, "model", None)   # (DetectMultiBackend wraps the model)
            if not hasattr(self.target, "infer_dtype"):
                raise TypeError("half= / dtype= need a yolov3_amd model (DetectionModel, or a DetectMultiBackend around one)")

    def __enter__(self):
        if self.target is not None:
            self.saved = self.target.__dict__.get("infer_dtype", self)
            self.target.infer_dtype = self.dtype
        return self.dtype

    def __exit__(self, *exc):
        if self.target is not None:
            if self.saved is self:
                self.target.__dict__.pop("infer_dtype", None)
            else:
                self.target.infer_dtype = self.saved
        return False


def detect_batches(model, batches, conf_thres=0.25, iou_thres=0.45, classes=None, agnostic=False, multi_label=False, max_det=300, half=False, dtype=None):
    """Throughput form of the `model(im)` -> `non_max_suppression(preds)` pair of reference val.py:364-376 / detect.py:196-200
    over a stream of batches: the NMS of batch i (a chain of small launches ending in the one device->host copy of the counts)
    runs on a second HIP stream while the forward of batch i+1 fills the CUs on the current stream.  Yields, in order and one
    batch late, the list of (n, 6) detections of every batch -- the same tensors the sequential pair returns.  `half` / `dtype`: run the forwards in that
    precision from the parameters as they are (fp32 masters stay fp32); floating batches are cast to it, as DetectMultiBackend(fp16=True).forward does."""
    from .general import non_max_suppression

    cur = torch.cuda.current_stream()
    side = torch.cuda.Stream(device=cur.device)
    pending = None

    def finish(p):
        pred, ev = p
        with torch.cuda.stream(side):
            side.wait_event(ev)
            dets = non_max_suppression(pred, conf_thres, iou_thres, classes, agnostic, multi_label, max_det=max_det)
        for d in dets:
            d.record_stream(cur)  # allocated on the side stream, consumed by the caller on the current one
        cur.wait_stream(side)
        return dets

    scope = _infer_dtype(model, half, dtype)
    for x in batches:
        with scope as dt:   # (per forward: a generator must not leave the model changed between its yields)
            if dt is not None and x.is_floating_point() and x.dtype != dt:
                x = x.to(dt)
            out = model(x)
        pred = out[0] if isinstance(out, (list, tuple)) else out
        ev = torch.cuda.Event()
        ev.record(cur)
        if pending is not None:
            yield finish(pending)
        pending = (pred, ev)
    if pending is not None:
        yield finish(pending)


def run_batches(model, batches, nc, conf_thres=0.001, iou_thres=0.6, max_det=300, single_cls=False, confusion=False, half=False, dtype=None):
    """The validation loop of reference val.py:351-428 over ``(im, targets, shapes)`` triples in the reference dataloader's format: im (bs, 3, h, w)
    (uint8 is scaled by 1 / 255 like val.py:358-359), targets (nl, 6) [image, class, x, y, w, h] normalised and grouped by image, shapes[i] =
    ((h0, w0), ((h / h0, w / w0), (pad_w, pad_h))).  The post-processing of batch i (NMS, scale_boxes, labels to native space, process_batch, the
    statistics and optionally the confusion matrix) runs on a second HIP stream while the forward of batch i + 1 fills the CUs, as in `detect_batches`;
    its only device->host copy is the NMS counts.  `half` (`dtype`): validate in float16 (that dtype) from the parameters as they are -- the reference's
    ``validate.run(model=ema.ema, half=amp)`` (train.py:445) without casting the averaged fp32 weights to half and back.  Returns ((mp, mr, map50, map), maps, stats[, confusion_matrix]) with `stats` the `ValStats` of the run."""
    from . import ops
    from .general import _gain_pad, non_max_suppression_batched
    from .metrics import ConfusionMatrix, ValStats

    cur = torch.cuda.current_stream()
    dev = cur.device
    side = torch.cuda.Stream(device=dev)
    iouv = torch.linspace(0.5, 0.95, 10, device=dev)
    stats = ValStats(nc, iouv, dev)
    cm = ConfusionMatrix(nc) if confusion else None
    scope = _infer_dtype(model, half, dtype)
    dtype = scope.dtype or getattr(model, "infer_dtype", None) or next(model.parameters()).dtype
    pending = None

    def finish(p):
        pred, ev, targets, shapes, hw = p
        bs = pred.shape[0]
        with torch.cuda.stream(side):
            side.wait_event(ev)
            rows, counts, counts_list = non_max_suppression_batched(pred, conf_thres, iou_thres, None, single_cls, True, max_det)
            if single_cls:
                rows[:, :, 5] = 0
            tab = []
            for i in range(bs):
                gain, px, py = _gain_pad(hw, shapes[i][0], shapes[i][1])
                tab.append([gain, px, py, float(shapes[i][0][1]), float(shapes[i][0][0])])
            params = torch.tensor(tab, dtype=torch.float32).to(dev, non_blocking=True)
            ops.scale_boxes_raw(rows, rows.stride(0), rows.stride(1), counts, bs, rows.shape[1], params)
            labels, offs = ops.labels_to_native(targets, bs, hw[1], hw[0], params)
            correct = process_batch_batched(rows, counts, labels, offs, iouv)
            stats.update(rows, counts, counts_list, correct, labels, offs)
            if cm is not None:
                cm.process_batch_batched(rows, counts, labels, offs)
        cur.wait_stream(side)

    for im, targets, shapes in batches:
        im = im.to(dev, non_blocking=True)
        if im.dtype == torch.uint8:
            im = im.to(dtype) / 255
        elif im.dtype != dtype:
            im = im.to(dtype)
        targets = targets.to(dev, torch.float32, non_blocking=True).contiguous()
        with scope:
            out = model(im)
        pred = out[0] if isinstance(out, (list, tuple)) else out
        ev = torch.cuda.Event()
        ev.record(cur)
        if pending is not None:
            finish(pending)
        pending = (pred, ev, targets, shapes, tuple(im.shape[2:]))
    if pending is not None:
        finish(pending)
    res = stats.results()
    return (res, stats.maps(nc), stats, cm) if confusion else (res, stats.maps(nc), stats)
