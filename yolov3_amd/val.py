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


def _engine_model(model):
    """the model the engine runs: `model` itself (a DetectionModel, an Ensemble), or the one a DetectMultiBackend wraps; None if there is none"""
    from .experimental import Ensemble

    if hasattr(model, "infer_dtype") or isinstance(model, Ensemble):
        return model
    inner = getattr(model, "model", None)
    return inner if hasattr(inner, "infer_dtype") or isinstance(inner, Ensemble) else None


class _infer_dtype:
    """``with _infer_dtype(model, half, dtype):`` -- the model's inference plans run in `dtype` (half: float16) inside the block, whatever its parameters are: fp32
    masters are read as they are and rounded once when the filter banks are packed (no ``model.half()`` ... ``model.float()`` round trip, reference val.py).
    Neither given: the block changes nothing.  An Ensemble: set on, and restored for, every member."""

    def __init__(self, model, half=False, dtype=None):
        from .experimental import Ensemble

        self.dtype = dtype if dtype is not None else (torch.float16 if half else None)
        self.targets = []
        if self.dtype is not None:
            inner = _engine_model(model)   # (DetectMultiBackend wraps the model)
            self.targets = list(inner) if isinstance(inner, Ensemble) else [inner]
            if not self.targets or not all(hasattr(t, "infer_dtype") for t in self.targets):
                raise TypeError("half= / dtype= need a yolov3_amd model (DetectionModel or Ensemble, or a DetectMultiBackend around one)")

    def __enter__(self):
        self.saved = [t.__dict__.get("infer_dtype", self) for t in self.targets]
        for t in self.targets:
            t.infer_dtype = self.dtype
        return self.dtype

    def __exit__(self, *exc):
        for t, saved in zip(self.targets, self.saved):
            if saved is self:
                t.__dict__.pop("infer_dtype", None)
            else:
                t.infer_dtype = saved
        return False


def _plan_dtype(model, scope):
    """the dtype the forwards inside `scope` run in"""
    from .experimental import Ensemble

    inner = _engine_model(model)
    first = inner[0] if isinstance(inner, Ensemble) and len(inner) else model
    return scope.dtype or getattr(first, "infer_dtype", None) or next(model.parameters()).dtype


def detect_batches(model, batches, conf_thres=0.25, iou_thres=0.45, classes=None, agnostic=False, multi_label=False, max_det=300, half=False, dtype=None, augment=False):
    """Throughput form of the `model(im)` -> `non_max_suppression(preds)` pair of reference val.py:364-376 / detect.py:196-200
    over a stream of batches: the NMS of batch i (a chain of small launches ending in the one device->host copy of the counts)
    runs on a second HIP stream while the forward of batch i+1 fills the CUs on the current stream.  Yields, in order and one
    batch late, the list of (n, 6) detections of every batch -- the same tensors the sequential pair returns.  `half` / `dtype`: run the forwards in that
    precision from the parameters as they are (fp32 masters stay fp32); floating batches are cast to it, as DetectMultiBackend(fp16=True).forward does.
    `augment`: ``model(x, augment=True)``, test-time augmentation (detect.py --augment).  `model` may be an Ensemble."""
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
            out = model(x, augment=True) if augment else model(x)
        pred = out[0] if isinstance(out, (list, tuple)) else out
        ev = torch.cuda.Event()
        ev.record(cur)
        if pending is not None:
            yield finish(pending)
        pending = (pred, ev)
    if pending is not None:
        yield finish(pending)


def run_batches(model, batches, nc, conf_thres=0.001, iou_thres=0.6, max_det=300, single_cls=False, confusion=False, half=False, dtype=None, augment=False, save_hybrid=False,
                compute_loss=None, save_txt=False, save_conf=False, save_json=False, save_dir=None, class_map=None, jdict=None, anno_json=None, coco_img_ids=None):
    """The validation loop of reference val.py:351-428 over ``(im, targets, shapes)`` triples in the reference dataloader's format: im (bs, 3, h, w)
    (uint8 is scaled by 1 / 255 like val.py:358-359), targets (nl, 6) [image, class, x, y, w, h] normalised and grouped by image, shapes[i] =
    ((h0, w0), ((h / h0, w / w0), (pad_w, pad_h))).  The post-processing of batch i (NMS, scale_boxes, labels to native space, process_batch, the
    statistics and optionally the confusion matrix) runs on a second HIP stream while the forward of batch i + 1 fills the CUs, as in `detect_batches`;
    its only device->host copy is the NMS counts.  `half` (`dtype`): validate in float16 (that dtype) from the parameters as they are -- the reference's
    ``validate.run(model=ema.ema, half=amp)`` (train.py:445) without casting the averaged fp32 weights to half and back.
    `augment` (val.py:364): ``model(im, augment=True)``; ignored when `compute_loss` is given, as there.
    `save_hybrid` (val.py:372): the batch's labels enter NMS as a-priori rows.  The forward writes the prediction straight into a buffer with a tail window
    (engine.run_model's ``out=``), which y3_label_rows fills with the labels in pixels of the batch; the window is as high as the largest label count of one image when
    the loader's targets are on the CPU, as the whole batch's otherwise (all-zero rows are never candidates), so nothing more is read back.
    `compute_loss` (val.py:364-368; train.py:445-456 passes it every epoch): a ``ComputeLoss``; ``compute_loss(train_out, targets)[1]`` of every batch is summed on the
    device and read back once, and the first element of the result becomes the reference's 7-tuple (mp, mr, map50, map, box, obj, cls): the sums divided by
    the number of batches (val.py:449).  An Ensemble has no train output (None in the reference): TypeError.
    `save_txt` / `save_conf` (val.py:410-411): ``save_dir / "labels" / (stem + ".txt")`` per image with detections, `cls x y w h [conf]` normalised by the native size.
    `save_json` (val.py:412-413, 454-462): the COCO-JSON entries of the run, appended to `jdict` (the caller's list, or a new one) and dumped to ``save_dir /
    "predictions.json"`` (a str or Path: that file name inside `save_dir`) when there are any; `class_map[int(cls)]` is the category id (``list(range(1000))`` as val.py:344;
    ``outputs.coco80_to_coco91_class()`` for COCO).  With either flag the batches are the dataloader's own 4-tuples ``(im, targets, paths,
    shapes)`` and `save_dir` is required (ValueError before anything is launched); a 4-tuple is accepted without them too.  The boxes of a batch are converted by one launch
    after scale_boxes (outputs.save_txt_batched / save_json_batched) and reach the host in one copy per flag; the metrics do not change.
    `anno_json` (val.py:464-477; needs `save_json`, ValueError otherwise): the COCO annotation file (a path, its dict, or a `coco_eval.CocoGroundTruth` to parse and upload it
    once for many runs).  After the dump the jdict is evaluated on the device (`coco_eval.CocoEval`: pycocotools' bbox AP / AR without pycocotools); `map` and `map50` of the
    results tuple become its ``stats[0]`` and ``stats[1]``, the base value of `maps` the new `map` (val.py:486), and the `CocoResult` is kept as ``stats.coco`` (None when
    there was nothing to evaluate).  `coco_img_ids`: the images to evaluate -- None: every image of the file; ``"seen"``: ``int(Path(p).stem)`` of the paths that went through
    the run (val.py:473); or a list of ids.  With ``anno_json=None`` nothing changes.
    Returns ((mp, mr, map50, map[, box, obj, cls]), maps, stats[, confusion_matrix]) with `stats` the `ValStats` of the run."""
    import itertools
    import json
    from pathlib import Path

    from . import ops, outputs
    from .experimental import Ensemble
    from .general import _gain_pad, non_max_suppression_batched
    from .metrics import ConfusionMatrix, ValStats

    saving = bool(save_txt or save_json)
    if anno_json is not None:
        if not save_json:
            raise ValueError("anno_json needs save_json: the COCO evaluation reads the run's COCO-JSON entries")
        if isinstance(anno_json, (str, Path)) and not Path(anno_json).is_file():
            raise FileNotFoundError(f"anno_json: {anno_json} does not exist")
    if saving:   # (before any device work: a wrong call must not cost a forward)
        if save_dir is None:
            raise ValueError("save_txt / save_json need save_dir")
        save_dir = Path(save_dir)
        batches = iter(batches)
        first = next(batches, None)
        if first is not None and len(first) != 4:
            raise ValueError("save_txt / save_json need the dataloader's 4-tuples (im, targets, paths, shapes): the file names come from the paths")
        batches = itertools.chain(() if first is None else (first,), batches)
        (save_dir / "labels" if save_txt else save_dir).mkdir(parents=True, exist_ok=True)   # val.py:279
        class_map = list(range(1000)) if class_map is None else class_map
        jdict = [] if jdict is None else jdict
    inner = _engine_model(model)
    if compute_loss is not None:
        if isinstance(inner, Ensemble):
            raise TypeError("compute_loss needs the raw head outputs of one model: an Ensemble's train output is None (reference models/experimental.py:85)")
        augment = False   # val.py:364: `model(im) if compute_loss else (model(im, augment=augment), None)`
    if save_hybrid and inner is None:
        raise TypeError("save_hybrid needs a yolov3_amd model (DetectionModel or Ensemble, or a DetectMultiBackend around one)")
    cur = torch.cuda.current_stream()
    dev = cur.device
    side = torch.cuda.Stream(device=dev)
    iouv = torch.linspace(0.5, 0.95, 10, device=dev)
    stats = ValStats(nc, iouv, dev)
    cm = ConfusionMatrix(nc) if confusion else None
    scope = _infer_dtype(model, half, dtype)
    dtype = _plan_dtype(model, scope)
    loss = torch.zeros(3, device=dev) if compute_loss is not None else None
    pending, seen, seen_paths = None, 0, []

    def finish(p):
        pred, ev, targets, shapes, hw, tail, paths = p
        bs = pred.shape[0]
        with torch.cuda.stream(side):
            side.wait_event(ev)
            tab = []
            for i in range(bs):
                gain, px, py = _gain_pad(hw, shapes[i][0], shapes[i][1])
                tab.append([gain, px, py, float(shapes[i][0][1]), float(shapes[i][0][0])])
            params = torch.tensor(tab, dtype=torch.float32).to(dev, non_blocking=True)
            labels, offs = ops.labels_to_native(targets, bs, hw[1], hw[0], params)
            if tail is not None:   # the a-priori rows behind the model's own, in pixels of the batch (val.py:371-372)
                ops.label_rows(pred, tail[0], tail[1], targets, offs, hw[1], hw[0])
            rows, counts, counts_list = non_max_suppression_batched(pred, conf_thres, iou_thres, None, single_cls, True, max_det)
            if single_cls:
                rows[:, :, 5] = 0
            ops.scale_boxes_raw(rows, rows.stride(0), rows.stride(1), counts, bs, rows.shape[1], params)
            if save_txt:   # val.py:410-413 on predn, the native-space rows (the class column already zeroed under single_cls)
                outputs.save_txt_batched(rows, (counts, counts_list), [s[0] for s in shapes], paths, save_dir / "labels", save_conf)
            if save_json:
                outputs.save_json_batched(rows, (counts, counts_list), paths, jdict, class_map)
            correct = process_batch_batched(rows, counts, labels, offs, iouv)
            stats.update(rows, counts, counts_list, correct, labels, offs)
            if cm is not None:
                cm.process_batch_batched(rows, counts, labels, offs)
        cur.wait_stream(side)

    for batch in batches:
        if saving and len(batch) != 4:
            raise ValueError("save_txt / save_json need the dataloader's 4-tuples (im, targets, paths, shapes)")
        im, targets, paths, shapes = batch if len(batch) == 4 else (batch[0], batch[1], None, batch[2])
        im = im.to(dev, non_blocking=True)
        if im.dtype == torch.uint8:
            im = im.to(dtype) / 255
        elif im.dtype != dtype:
            im = im.to(dtype)
        extra = 0
        if save_hybrid and targets.shape[0]:
            if targets.device.type == "cpu":   # the loader's own tensor: the largest label count of one image, counted on the host
                extra = int(torch.bincount(targets[:, 0].long().clamp_(0, im.shape[0])).max())
            else:
                extra = int(targets.shape[0])
        targets = targets.to(dev, torch.float32, non_blocking=True).contiguous()
        tail = None
        with scope:
            if extra and compute_loss is None:
                rows = _pred_rows(inner, im, augment)
                pred = torch.empty(im.shape[0], rows + extra, (inner[0] if isinstance(inner, Ensemble) else inner).model[-1].no, dtype=dtype, device=dev)
                inner._predict_into(im, (pred, 0), augment)
                tail = (rows, extra)
            else:
                out = model(im, augment=True) if augment else model(im)
                pred = out[0] if isinstance(out, (list, tuple)) else out
                if compute_loss is not None:
                    with torch.no_grad():
                        loss += compute_loss(out[1], targets)[1]   # box, obj, cls (val.py:368), with the normalised targets
                if extra:   # (compute_loss keeps the raw tensors, which the windowed forward does not write: the prediction is widened by one copy instead)
                    wide = torch.empty(pred.shape[0], pred.shape[1] + extra, pred.shape[2], dtype=pred.dtype, device=dev)
                    wide[:, : pred.shape[1]].copy_(pred)
                    pred, tail = wide, (pred.shape[1], extra)
        ev = torch.cuda.Event()
        ev.record(cur)
        if pending is not None:
            finish(pending)
        pending = (pred, ev, targets, shapes, tuple(im.shape[2:]), tail, paths)
        seen += 1
        if anno_json is not None:
            seen_paths.extend(paths)
    if pending is not None:
        finish(pending)
    if save_json and len(jdict):   # val.py:454-462, without the pycocotools evaluation behind it
        with open(save_dir / ("predictions.json" if save_json is True else Path(save_json).name), "w") as f:
            json.dump(jdict, f)
    res, maps = stats.results(), stats.maps(nc)
    if anno_json is not None:
        stats.coco = None
        if len(jdict):   # val.py:464-477 on the device: map, map50 = eval.stats[:2]
            import numpy as np

            from .coco_eval import CocoEval, CocoGroundTruth

            gt = anno_json if isinstance(anno_json, CocoGroundTruth) else CocoGroundTruth(anno_json, dev)
            img_ids = [int(Path(p).stem) for p in seen_paths] if isinstance(coco_img_ids, str) and coco_img_ids == "seen" else coco_img_ids
            stats.coco = CocoEval(gt, img_ids).evaluate(jdict)
            coco_map, coco_map50 = (float(v) for v in stats.coco.stats[:2])
            res = (res[0], res[1], coco_map50, coco_map)
            maps = np.zeros(nc) + coco_map   # val.py:486-488: the new mean, then the loop's own AP of every class with labels
            if stats.n and stats._result[1]:
                ap, classes = stats.compute()[5], stats.compute()[6]
                for i, c in enumerate(classes):
                    maps[c] = ap[i].mean()
    if loss is not None:
        res = (*res, *(loss.cpu() / max(seen, 1)).tolist())
    return (res, maps, stats, cm) if confusion else (res, maps, stats)


def _pred_rows(model, im, augment):
    """rows of `model(im, augment)[0]`, on the host (engine.pred_rows; an Ensemble: the sum over its members)"""
    from .engine import pred_rows

    return model.pred_rows(im.shape[2], im.shape[3], augment) if hasattr(model, "pred_rows") else pred_rows(model, im.shape[2], im.shape[3], augment)
