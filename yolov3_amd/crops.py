"""The second-stage classifier of the detect loop on the device (reference utils/general.py:827-859 apply_classifier; its hook at detect.py:202-203).

    x = non_max_suppression(pred, conf_thres, iou_thres)              # a list of (n, 6) DEVICE tensors, letterboxed space
    x = apply_classifier(x, classifier, im, im0s)                      # the reference's signature and result
    rows, counts_t, counts = apply_classifier_batched(*non_max_suppression_batched(pred), classifier, im.shape[2:], DeviceImages(im0s))

The reference cuts every detection out of its native image on the host -- one NumPy slice, one cv2.resize to 224 x 224 and one float conversion per detection, one
classifier call per image -- and needs the detections on the host before the first crop is cut.  Here the native images are uploaded once (DeviceImages: the arena
and the 32-byte records of dataset.py) and csrc/crops.hip does the rest in four launches for the whole batch: y3_classifier_boxes (xyxy2xywh, rectangle to square,
`* 1.3 + 30`, xywh2xyxy, .long() into a table of its own), y3_scale_boxes on that table (the one definition of scale_boxes), y3_crop_resize (every crop resized to
(S, S), RGB, CHW, divided by 255, in the classifier's dtype) and, behind the classifier, y3_keep_matching (the rows whose class the classifier confirms, compacted in
order).  N = sum(counts) is known on the host from the NMS, so nothing is read back before the classifier runs; afterwards ONE copy brings the bs new counts and the
status word.

Differences from the reference, all deliberate:
  * ONE classifier call per batch where the reference makes one per image: the same result for any model whose output rows do not depend on the rest of the batch;
  * a crop that cannot be cut -- an empty cutout, a box outside its image -- is written as zeros and counted in a device status word, and a non-zero word raises
    ValueError naming the count, where the reference's cv2.resize raises cv2.error on the first empty cutout;
  * CPU tensors raise (ops.require_gpu): there is no CPU path;
  * cv2 is not here: the resize is the 8-bit INTER_LINEAR arithmetic restated for y3_letterbox_u8 (csrc/y3_resize_u8.h), which no cv2 build has checked.
"""
from __future__ import annotations

import numpy as np
import torch

from . import ops
from .dataset import _ALIGN, _RECORD, _device, _upload, _upload_arena
from .general import _gain_pad


class DeviceImages:
    """A list of (h, w, 3) uint8 images of any sizes (BGR, the caller's im0s), uploaded once: one arena, one record table.  `.shapes`: the (h, w) list."""

    def __init__(self, ims, device="cuda"):
        ims = [ims] if isinstance(ims, np.ndarray) else list(ims)
        if not ims:
            raise ValueError("DeviceImages: no image")
        for i, im in enumerate(ims):
            if not isinstance(im, np.ndarray) or im.dtype != np.uint8 or im.ndim != 3 or im.shape[2] != 3 or im.shape[0] < 1 or im.shape[1] < 1:
                raise TypeError(f"DeviceImages: image {i} is not an (h, w, 3) uint8 array")
        self.device = _device(device)
        ims = [np.ascontiguousarray(im) for im in ims]
        self.n, self.shapes = len(ims), [tuple(int(v) for v in im.shape[:2]) for im in ims]
        rec = np.zeros(self.n, dtype=_RECORD)
        offsets = np.zeros(self.n + 1, dtype=np.int64)
        for j, im in enumerate(ims):
            offsets[j + 1] = offsets[j] + -(-im.nbytes // _ALIGN) * _ALIGN
            rec[j] = (offsets[j], im.shape[0], im.shape[1], 0, 0, 0, 0)
        self.arena = _upload_arena(ims, offsets, int(offsets[-1]), self.device)
        self.records = _upload(rec.view(np.uint8).reshape(-1), self.device)

    def __len__(self):
        return self.n


def _check(what, rows, counts_t, counts, img1_shape, images, size, dtype):
    """Every refusal the host can make, in one place and ahead of any upload or launch -> (bs, max_det, N, the (h, w) of every image)."""
    if not isinstance(rows, torch.Tensor) or rows.dtype != torch.float32 or rows.dim() != 3 or rows.shape[2] != 6 or not rows.is_contiguous():
        raise TypeError(f"{what} expects the contiguous (bs, max_det, 6) fp32 rows of non_max_suppression_batched")
    bs, max_det = int(rows.shape[0]), int(rows.shape[1])
    if not isinstance(counts_t, torch.Tensor) or counts_t.dtype != torch.int32 or tuple(counts_t.shape) != (bs,):
        raise TypeError(f"{what} expects the ({bs},) int32 device counts of non_max_suppression_batched")
    counts = [int(c) for c in counts]
    if len(counts) != bs or any(c < 0 or c > max_det for c in counts):
        raise ValueError(f"{what}: the host counts {counts} do not describe {bs} images of at most {max_det} detections")
    if len(img1_shape) != 2 or min(img1_shape) < 1:
        raise ValueError(f"{what}: img1_shape = {tuple(img1_shape)}; the (h, w) of the letterboxed batch")
    if isinstance(size, bool) or not isinstance(size, (int, np.integer)) or not 1 <= size <= ops.CROP_MAX_SIZE:
        raise ValueError(f"{what}: size = {size!r}; crops are 1 .. {ops.CROP_MAX_SIZE} pixels on a side")
    if dtype not in ops.CROP_DTYPES:
        raise TypeError(f"{what} writes float16 / bfloat16 / float32 crops, not {dtype}")
    if isinstance(images, DeviceImages):
        shapes = images.shapes
    else:
        images = [images] if isinstance(images, np.ndarray) else list(images)
        for i, im in enumerate(images):
            if not isinstance(im, np.ndarray) or im.dtype != np.uint8 or im.ndim != 3 or im.shape[2] != 3:
                raise TypeError(f"{what}: image {i} is not an (h, w, 3) uint8 array")
        shapes = [im.shape[:2] for im in images]
    if len(shapes) != bs:
        raise ValueError(f"{what}: {len(shapes)} images for the detections of {bs}")
    ops.require_gpu(rows, what)
    ops.require_gpu(counts_t, what)
    return bs, max_det, counts, shapes


def _crops(what, rows, counts_t, counts, img1_shape, images, size, dtype, gain, pad, square):
    bs, max_det, counts, shapes = _check(what, rows, counts_t, counts, img1_shape, images, size, dtype)
    dev = rows.device
    n = sum(counts)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    prefix_host = np.zeros(bs, dtype=np.int64)
    np.cumsum(np.asarray(counts[:-1], dtype=np.int64), out=prefix_host[1:])
    prefix = _upload(prefix_host, dev)
    if n == 0:   # nothing to cut: no upload of the images, no launch
        return torch.empty(0, 3, size, size, dtype=dtype, device=dev), torch.zeros(bs, max_det, 4, dtype=torch.float32, device=dev), prefix, status, None
    if not isinstance(images, DeviceImages):
        images = DeviceImages(images, dev)
    boxes = ops.classifier_boxes(rows, counts_t, gain, pad, square)
    tab = []
    for h0, w0 in shapes:   # the per-image parameters as scale_boxes_batched forms them
        g, px, py = _gain_pad(img1_shape, (h0, w0), None)
        tab.append([g, px, py, float(w0), float(h0)])
    ops.scale_boxes_raw(boxes, boxes.stride(0), 4, counts_t, bs, max_det, _upload(np.asarray(tab, dtype=np.float32), dev))
    crops, status = ops.crop_resize(images.arena, images.records, boxes, counts_t, prefix, n, int(size), dtype, status)
    return crops, boxes, prefix, status, images


def classifier_crops(rows, counts_t, counts, img1_shape, images, size=224, dtype=torch.float32, gain=1.3, pad=30, square=True):
    """The crops apply_classifier feeds its model, for a whole batch: `rows` (bs, max_det, 6), `counts_t` and `counts` the result of non_max_suppression_batched in
    the letterboxed space of `img1_shape` (h, w), `images` a DeviceImages or a list of (h, w, 3) uint8 BGR arrays (uploaded for the call) ->
    (crops DEVICE (N, 3, size, size) `dtype`, N = sum(counts), image by image; boxes DEVICE fp32 (bs, max_det, 4), the padded squares in native pixels; prefix DEVICE
    int64 (bs,): crop k of image i is crops[prefix[i] + k]; status DEVICE int32 (1,): the crops that could not be cut and are zeros).  Nothing is read back."""
    return _crops("classifier_crops", rows, counts_t, counts, img1_shape, images, size, dtype, gain, pad, square)[:4]


def _classes(model, crops):
    pred = model(crops)
    if not isinstance(pred, torch.Tensor) or pred.dim() != 2 or pred.shape[0] != crops.shape[0]:
        raise TypeError("apply_classifier: the classifier must return one row of logits per crop")
    return pred.argmax(1).contiguous()


def apply_classifier_batched(rows, counts_t, counts, model, img1_shape, images, size=224, dtype=None):
    """apply_classifier in the convention of non_max_suppression_batched: -> (rows (bs, max_det, 6) with every image's kept rows first, in order, then zeros;
    counts_t DEVICE int32 (bs,); counts, the host list).  `model` is called once, on all crops, in `dtype` (None: the dtype of its first parameter, float32 for a
    model without parameters).  ValueError when a crop could not be cut."""
    what = "apply_classifier"
    if dtype is None:
        p = next(iter(model.parameters()), None) if hasattr(model, "parameters") else None
        dtype = p.dtype if p is not None else torch.float32
    crops, boxes, prefix, status, images = _crops(what, rows, counts_t, counts, img1_shape, images, size, dtype, 1.3, 30, True)
    if crops.shape[0] == 0:
        return rows.clone(), counts_t.clone(), [0] * rows.shape[0]
    kept, kept_counts = ops.keep_matching(rows, counts_t, prefix, _classes(model, crops), boxes, images.arena, images.records)
    back = torch.cat((kept_counts, status)).tolist()   # ONE copy: the bs new counts and the status word
    if back[-1]:
        raise ValueError(f"{what}: {back[-1]} of {crops.shape[0]} crops could not be cut (an empty cutout or a box outside its image)")
    return kept, kept_counts, back[:-1]


def apply_classifier(x, model, img, im0):
    """Drop-in for reference utils/general.py:827: `x` a list with one (n, 6) DEVICE tensor per image (entries may be None or empty), `img` the letterboxed batch or
    its (h, w), `im0` one array, a list of arrays or a DeviceImages -> the list with every image's rows the classifier confirms (None stays None)."""
    what = "apply_classifier"
    x = list(x)
    img1_shape = tuple(img.shape[2:]) if isinstance(img, torch.Tensor) else tuple(int(v) for v in img)
    live = [d for d in x if d is not None and len(d)]
    for d in live:
        if not isinstance(d, torch.Tensor) or d.dim() != 2 or d.shape[1] != 6 or d.dtype != torch.float32:
            raise TypeError(f"{what} expects (n, 6) fp32 detections")
        ops.require_gpu(d, what)
    if not live:
        return x
    counts = [0 if d is None else len(d) for d in x]
    rows = torch.zeros(len(x), max(counts), 6, dtype=torch.float32, device=live[0].device)
    for i, d in enumerate(x):
        if counts[i]:
            rows[i, : counts[i]] = d
    counts_t = _upload(np.asarray(counts, dtype=np.int32), rows.device)
    kept, _, new = apply_classifier_batched(rows, counts_t, counts, model, img1_shape, im0)
    return [kept[i, : new[i]] if counts[i] else d for i, d in enumerate(x)]
