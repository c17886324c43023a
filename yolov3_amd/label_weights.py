"""Class and image weights for --image-weights training on the device (reference utils/general.py:543-568, train.py:333 and :360-363).

    model.class_weights = labels_to_class_weights(dataset.labels, nc).to(device) * nc           # train.py:333
    cw = model.class_weights.cpu().numpy() * (1 - maps) ** 2 / nc                               # the epoch prologue, train.py:360-363
    dataset.indices = image_weight_indices(table, cw)                                           # labels_to_image_weights + random.choices in one call

The reference runs one np.bincount per image on the host, every epoch.  Here a LabelTable uploads the class column of every label once; the class histogram, the
per-image weighted sums, the cumulative weights and the k searches of random.choices run through csrc/label_weights.hip (y3_label_histogram / y3_image_weights /
y3_weighted_choices).  The host keeps what is not arithmetic over the labels: the nc-element tail of labels_to_class_weights, in NumPy in the reference's order (so
the class weights are the reference's bit for bit), and the random draws -- one random.random() per sample from Python's global generator, what random.choices
consumes, so a seeded run leaves the stream where the reference leaves it.

Differences from the reference, all deliberate:
  * a class id (truncated toward zero, as astype(int)) below 0 or at or above nc raises ValueError when the table is built (np.bincount raises for a negative id
    and silently grows the vector for a large one, after which labels_to_image_weights fails to broadcast);
  * class weights that are not finite raise ValueError;
  * image weights are the fp64 sum of class_weights[id] over the image's labels in the kernel's fixed order, not NumPy's sum over the nc products: equal within
    (nc + labels of the image) 2^-52 relative for weights of one sign, and run-to-run bit-identical; likewise the cumulative weights behind the indices;
  * there is no CPU path.
"""
from __future__ import annotations

import random

import numpy as np
import torch

from . import ops

_STATUS = {1: "Total of weights must be greater than zero", 2: "Total of weights must be finite"}   # random.choices' own messages


def _device(device, what: str) -> torch.device:
    if device is None and not torch.cuda.is_available():
        raise RuntimeError(f"{what}: no CPU / PyTorch fallback; the yolov3_amd hot path runs only on an MI355X (HIP) device.")
    device = torch.device(device if device is not None else "cuda")
    ops.require_gpu(torch.empty(0, device=device), what)
    return device


def _upload(a: np.ndarray, device) -> torch.Tensor:
    """every host -> device copy of this module"""
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _download(t: torch.Tensor) -> torch.Tensor:
    """every device -> host copy of this module"""
    return t.cpu()


class LabelTable:
    """The class column of dataset.labels (a list of (m, 5) arrays [class, x, y, w, h], m may be 0) on the device: one contiguous fp32 array of the N class ids and
    n + 1 segment offsets, uploaded once.  .n images, .N labels, .nc classes, .class_counts() the int64 histogram."""

    def __init__(self, labels, nc, device=None):
        device = _device(device, "LabelTable")
        self.nc, self.n = int(nc), len(labels)
        if self.n < 1:
            raise ValueError("LabelTable: no images")
        if self.nc < 1:
            raise ValueError(f"LabelTable: nc = {nc}")
        cols = [np.asarray(x).reshape(-1, 5)[:, 0] for x in labels]
        offsets = np.zeros(self.n + 1, dtype=np.int64)
        np.cumsum([len(c) for c in cols], out=offsets[1:])
        self.N = int(offsets[-1])
        cls = np.concatenate(cols) if self.N else np.zeros(0, dtype=np.float32)
        if cls.dtype != np.float32:   # the dataloader's labels are fp32; any other type is truncated in its own precision first: an integer below 2^24 is exact in fp32
            cls = np.trunc(cls.astype(np.float64)).astype(np.float32)
        self.device = device
        self.cls = _upload(cls, device)
        self.offsets = _upload(offsets, device)
        counts = _download(ops.label_histogram(self.cls, self.nc)).numpy().astype(np.int64)   # the one read: nc counts and the error word
        if counts[-1]:
            raise ValueError(f"LabelTable: {int(counts[-1])} of {self.N} labels have a class id outside [0, {self.nc})")
        self._counts = counts[:-1]

    def class_counts(self) -> np.ndarray:
        """labels per class, int64 (nc,): np.bincount(classes, minlength=nc)"""
        return self._counts.copy()

    def class_weights_device(self, class_weights) -> torch.Tensor:
        cw = np.asarray(class_weights, dtype=np.float64).reshape(self.nc)   # (a size other than nc fails here, as the reference's reshape(1, nc) does)
        if not np.isfinite(cw).all():
            raise ValueError("class_weights must be finite")
        return _upload(cw, self.device)

    def image_weights(self, class_weights) -> torch.Tensor:
        """iw[i] = sum_c class_weights[c] * count[i][c] -> DEVICE fp64 (n,)"""
        return ops.image_weights(self.cls, self.offsets, self.class_weights_device(class_weights))


def _table(labels, nc, device) -> LabelTable:
    return labels if isinstance(labels, LabelTable) else LabelTable(labels, nc, device)


def labels_to_class_weights(labels, nc=80, *, device=None):
    """Class weights from the training labels (reference utils/general.py:543-561) -> fp32 CPU tensor (nc,), the reference's bit for bit.  labels: dataset.labels or a
    LabelTable (whose nc is used)."""
    if not isinstance(labels, LabelTable) and labels[0] is None:   # no labels loaded
        return torch.Tensor()
    weights = _table(labels, nc, device).class_counts()   # occurrences per class
    weights[weights == 0] = 1   # replace empty bins with 1
    weights = 1 / weights       # number of targets per class
    weights /= weights.sum()    # normalize
    return torch.from_numpy(weights).float()


def labels_to_image_weights(labels, nc=80, class_weights=np.ones(80), *, device=None):  # noqa: B008
    """Image weights from the labels and class weights (reference utils/general.py:564-568) -> np.float64 (n,)"""
    return _download(_table(labels, nc, device).image_weights(class_weights)).numpy()


def image_weight_indices(table: LabelTable, class_weights, k=None, device_weights=False):
    """The --image-weights epoch prologue (train.py:362-363) in one call: random.choices(range(n), weights=labels_to_image_weights(labels, nc, class_weights), k=k)
    -> a list of k ints (k = table.n by default); with device_weights=True also the image weights, DEVICE fp64 (n,).  The k uniforms are drawn with random.random();
    raises random.choices' ValueError, with the generator left untouched, when the total of the weights is not positive or not finite."""
    if not isinstance(table, LabelTable):
        raise TypeError("image_weight_indices expects a LabelTable")
    cw = table.class_weights_device(class_weights)
    k = table.n if k is None else int(k)
    state = random.getstate()
    u = _upload(np.array([random.random() for _ in range(k)], dtype=np.float64), table.device)
    iw = ops.image_weights(table.cls, table.offsets, cw)
    out = _download(ops.weighted_choices(iw, u)).tolist()   # the one read: k indices and the status word
    status = out.pop()
    if status:
        random.setstate(state)   # random.choices raises before it draws
        raise ValueError(_STATUS[status])
    return (out, iw) if device_weights else out
