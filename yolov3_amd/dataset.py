"""A cached dataset kept on the device and iterated without a host loader (reference utils/dataloaders.py:548-570, 659-735, 825-830; train.py:299-312, val.py:351-360).

    ds = DeviceDataset(images, labels, img_size=640, batch_size=32, stride=32, pad=0.5, rect=True)      # or DeviceDataset.from_dataset(val_loader.dataset, batch_size=32)
    for im, targets, paths, shapes in ds: ...                                                           # the reference loader's 4-tuple; im / targets are DEVICE tensors
    results, maps, stats = run_batches(model, ds, nc=80)

It is the `--cache ram` idea with the cache in HBM, for the augment=False path: the cached images are already resized by load_image, and the batch shapes of
dataloaders.py:548-570 make letterbox(auto=False, scaleup=False) take its pad-only branch (r == 1, cv2.resize is never called).  What is left per image -- a constant
114 border, transpose((2, 0, 1))[::-1], xywhn2xyxy / xyxy2xywhn on the labels, collate_fn -- runs through csrc/dataset.hip: one launch of y3_dataset_batch and one of
y3_dataset_targets per batch, no device -> host copy, and no host -> device copy either (the indices of a shuffled epoch are uploaded once by set_indices).

The host keeps what is not per-pixel or per-label work, computed once per image when the set is built: the aspect-ratio order and the batch shapes (rect_batch_shapes),
letterbox's top / left / (dw, dh), and the `paths` / `shapes` entries of the 4-tuple.

Differences from the reference, all deliberate:
  * an image that does not fit its batch shape raises ValueError (fitting it needs cv2.resize, which is not here);
  * a batch width that is no multiple of 16 raises ValueError (the kernel stores 16 bytes per lane; every stride-32 shape qualifies);
  * dtype=torch.float16 / bfloat16 / float32 yields batches already divided by 255: the fp32 IEEE quotient rounded once, what `im.to(dtype) / 255` gives;
  * there is no CPU path, no augmentation, no mosaic.

store="host" (this class and the two train-mode sets of augment.py) keeps the cache where the reference keeps it, in host memory, for a set that does not fit HBM: the
images in ONE pinned host tensor, and on the device a ring of two halves, each sized exactly for the worst batch of the set (ring_half_bytes) with its own copy of the
record table.  Per batch plan_slots names the unique images and their 16-byte aligned slots in a half, and one launch of y3_dataset_stage (csrc/dataset_stage.hip) copies
them from the host arena over PCIe and writes their records with the slots' offsets; y3_dataset_batch / y3_dataset_targets then read (half, its table) where they read
(arena, table): the batches are bit-identical.  prefetch=1 (the default under store="host"): when __iter__ hands out batch k, the stage of batch k + 1 is
already launched on a side stream the set owns and runs under the caller's step on batch k, ordered by events (HostStore); prefetch=0 stages inside get_batch on the
current stream; get_batch(k) out of turn always works.  This class reads nothing back per batch, so the
stage's status word (jobs the kernel skipped: none for a plan of this module) is read once, at the end of an epoch.  Refused before anything is pinned or uploaded: an
unknown store, prefetch not in (0, 1), prefetch=1 with store="device".
"""
from __future__ import annotations

import math
from typing import NamedTuple

import numpy as np
import torch

from . import ops

_RECORD = np.dtype(ops.Y3DatasetImage)   # y3_dataset_image as include/yolov3_hip.h declares it
_ALIGN = 16
_CHUNK = 64 << 20   # bytes of the pinned staging buffer
_DTYPES = (torch.uint8, torch.float16, torch.bfloat16, torch.float32)


def rect_batch_shapes(shapes_wh, img_size, batch_size, stride, pad):
    """The rectangular-batch layout of reference utils/dataloaders.py:528-570 -> (order, batch_index, batch_shapes): `order` the aspect-ratio sort of the images
    (h / w of `shapes_wh`, the (w, h) rows of dataset.shapes, ascending, NumPy's default argsort), `batch_index[j]` the batch of the j-th image of that order, and
    `batch_shapes` int (nb, 2): the (H, W) every image of a batch is letterboxed to -- [maxi, 1] for a batch of wide images, [1, 1 / mini] for one of tall images,
    [1, 1] otherwise, times img_size / stride, plus pad, rounded up, times stride."""
    s = np.asarray(shapes_wh)
    if s.ndim != 2 or s.shape[1] != 2 or len(s) < 1:
        raise ValueError("rect_batch_shapes expects the (n, 2) [w, h] shapes of at least one image")
    n = len(s)
    bi = np.floor(np.arange(n) / batch_size).astype(int)
    nb = bi[-1] + 1
    ar = s[:, 1] / s[:, 0]
    order = ar.argsort()
    ar = ar[order]
    shapes = [[1, 1]] * nb
    for i in range(nb):
        ari = ar[bi == i]
        mini, maxi = ari.min(), ari.max()
        if maxi < 1:
            shapes[i] = [maxi, 1]
        elif mini > 1:
            shapes[i] = [1, 1 / mini]
    return order, bi, np.ceil(np.array(shapes) * img_size / stride + pad).astype(int) * stride


class Layout(NamedTuple):
    """Where every image of the set goes, host values only: `order` (the constructor's images in the set's order), `batch` (n,) and `batch_shapes` (nb, 2) [H, W],
    per image of the set's order `top` / `left` (letterbox's border before the image) and `shapes`, the reference's ((h0, w0), ((h / h0, w / w0), (dw, dh)))."""

    order: np.ndarray
    batch: np.ndarray
    batch_shapes: np.ndarray
    top: np.ndarray
    left: np.ndarray
    shapes: list


def layout(hw, hw0, img_size, batch_size, stride=32, pad=0.0, rect=True, names=None, adopt=None) -> Layout:
    """The Layout of cached images of sizes `hw` (n, 2) [h, w] with original sizes `hw0` [h0, w0].  rect: sorted and shaped by rect_batch_shapes over the original
    sizes, or `adopt`ing (batch, batch_shapes) of a set that is in that order already; otherwise every batch is the square img_size.  top / left are
    letterbox's round(dh - 0.1) / round(dw - 0.1) on the halved paddings (Python's round).  ValueError for an image that does not fit its batch shape, and for a
    batch width that is no multiple of 16."""
    hw, hw0 = [(int(h), int(w)) for h, w in hw], [(int(h), int(w)) for h, w in hw0]
    n = len(hw)
    if rect and adopt is not None:
        order, batch, batch_shapes = np.arange(n), np.asarray(adopt[0]).astype(int), np.asarray(adopt[1]).astype(int).reshape(-1, 2)
        if not np.array_equal(batch, np.floor(np.arange(n) / batch_size).astype(int)) or len(batch_shapes) != batch[-1] + 1:
            raise ValueError(f"DeviceDataset: the dataset's batch index was not built for {n} images in batches of {batch_size}")
    elif rect:
        order, batch, batch_shapes = rect_batch_shapes([(w0, h0) for h0, w0 in hw0], img_size, batch_size, stride, pad)
    else:
        order, batch = np.arange(n), np.floor(np.arange(n) / batch_size).astype(int)
        batch_shapes = np.full((batch[-1] + 1, 2), int(img_size), dtype=int)
    bad = [int(w) for w in batch_shapes[:, 1] if w % 16]
    if bad:
        raise ValueError(f"DeviceDataset: the batch width {bad[0]} is not a multiple of 16")
    top, left, shapes = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32), []
    for j, i in enumerate(order):
        (h, w), (h0, w0) = hw[i], hw0[i]
        H, W = (int(v) for v in batch_shapes[batch[j]]) if rect else (int(img_size), int(img_size))
        if min(H / h, W / w) < 1.0:   # letterbox would scale down: r != 1
            raise ValueError(f"DeviceDataset: image {names[i] if names is not None else i} ({h}x{w}) does not fit its batch shape {H}x{W}; fitting it needs cv2.resize, "
                             "which is out of scope")
        dw, dh = (W - w) / 2, (H - h) / 2   # the padding, divided into 2 sides
        top[j], left[j] = round(dh - 0.1), round(dw - 0.1)
        shapes.append(((h0, w0), ((h / h0, w / w0), (dw, dh))))
    return Layout(order, batch, batch_shapes, top, left, shapes)


def _device(device) -> torch.device:
    what = "DeviceDataset"
    if device is None and not torch.cuda.is_available():
        raise RuntimeError(f"{what}: no CPU / PyTorch fallback; the yolov3_amd hot path runs only on an MI355X (HIP) device.")
    device = torch.device(device if device is not None else "cuda")
    if device.type != "cuda" or not torch.cuda.is_available():
        raise RuntimeError(f"{what}: device {device}; the yolov3_amd hot path runs only on an MI355X (HIP) device. There is no CPU / PyTorch fallback.")
    return device


def _upload(a: np.ndarray, device) -> torch.Tensor:
    """every small host -> device copy of this module"""
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _upload_arena(images, offsets, total: int, device) -> torch.Tensor:
    """the images back to back at their offsets -> one DEVICE uint8 arena, in chunks of whole images through one pinned staging buffer"""
    arena = torch.empty(total, dtype=torch.uint8, device=device)
    stage = torch.empty(max(_CHUNK, int(np.diff(offsets).max())), dtype=torch.uint8).pin_memory()   # (holds the largest image with its alignment gap)
    host = stage.numpy()
    i, n = 0, len(images)
    while i < n:
        start = int(offsets[i])
        j = i
        while j < n and int(offsets[j + 1]) - start <= host.size:
            a, b, c = int(offsets[j]) - start, int(offsets[j]) - start + images[j].nbytes, int(offsets[j + 1]) - start
            host[a:b] = images[j].reshape(-1)
            host[b:c] = 0   # the alignment gap behind the image
            j += 1
        size = int(offsets[j]) - start
        arena[start : start + size].copy_(stage[:size], non_blocking=True)
        torch.cuda.current_stream(device).synchronize()   # (the staging buffer is refilled next; the upload happens once per set)
        i = j
    return arena


STORES = ("device", "host")


def check_store(what: str, store, prefetch) -> int:
    """the refusals of the `store` / `prefetch` pair -> prefetch (None: 1 under store="host", else 0)"""
    if store not in STORES:
        raise ValueError(f"{what}: store = {store!r}; 'device' (the whole set in HBM) or 'host' (the set in pinned host memory, a batch at a time staged into HBM)")
    if prefetch is None:
        return 1 if store == "host" else 0
    if isinstance(prefetch, bool) or not isinstance(prefetch, (int, np.integer)) or prefetch not in (0, 1):
        raise ValueError(f"{what}: prefetch = {prefetch!r} (0: stage inside get_batch, 1: stage the next batch while this one is used)")
    if prefetch and store == "device":
        raise ValueError(f"{what}: prefetch = 1 with store = 'device': a resident set has nothing to stage")
    return int(prefetch)


def ring_half_bytes(slots, per_item: int, batch_size: int) -> int:
    """The bytes of one half of the ring: the worst batch of a set whose images take `slots` bytes (16-byte aligned sizes) when an item draws at most `per_item`
    images -- the sum of the min(n, per_item * batch_size) largest slots."""
    slots = np.asarray(slots, dtype=np.int64)
    k = min(len(slots), int(per_item) * int(batch_size))
    return int(np.sort(slots)[::-1][:k].sum())


def plan_slots(indices, slots, half_bytes: int):
    """Where the images of one batch go in a half of the ring, a pure function of the drawn indices -> (unique (m,) int64, offsets (m,) int64): every image once,
    in the order of its first draw, back to back at 16-byte aligned offsets.  ValueError for an index outside the set and for a batch that exceeds the half."""
    slots = np.asarray(slots, dtype=np.int64)
    unique = np.fromiter(dict.fromkeys(int(i) for i in indices), dtype=np.int64)
    if len(unique) and (unique.min() < 0 or unique.max() >= len(slots)):
        raise ValueError(f"plan_slots: image indices outside [0, {len(slots)})")
    ends = np.cumsum(slots[unique])
    if len(ends) and ends[-1] > half_bytes:
        raise ValueError(f"plan_slots: the {len(unique)} images of the batch take {int(ends[-1])} bytes, the ring half holds {int(half_bytes)} (items drawn for another set?)")
    return unique, ends - slots[unique]


def stage_jobs(unique, offsets, slots, chunk: int) -> np.ndarray:
    """the job table of y3_dataset_stage for a plan: int64 (m, 3) [image, slot offset, chunks of the jobs up to and including this one]"""
    jobs = np.zeros((len(unique), 3), dtype=np.int64)
    jobs[:, 0], jobs[:, 1] = unique, offsets
    np.cumsum(-(-np.asarray(slots, dtype=np.int64)[unique] // int(chunk)), out=jobs[:, 2])
    return jobs


class HostStore:
    """The images of a set in ONE pinned host tensor and a device ring of two halves, each with its own copy of the record table (a shared table would let the stage
    of batch k + 1 move the offset of an image that batch k's kernel is still reading).  `acquire` hands the consumer launches of a batch a half that holds its
    images -- the one `stage_ahead` filled on the store's side stream, else one filled now on the current stream -- and `release` marks their end.  Events order
    the two streams: a stage waits for the last consumers of the half it overwrites, the consumers wait for the stage.  `reserve(front)`: the bytes a batch's own records
    take in the pinned copy that carries the job table up (the train-mode sets: the item records and the copy-paste candidates)."""

    def __init__(self, images, offsets, rec, per_item, batch_size, device):
        n, total = len(images), int(offsets[-1])
        self.n, self.device, self.slots = n, device, np.diff(offsets).astype(np.int64)
        self.half_bytes = ring_half_bytes(self.slots, per_item, batch_size)
        self.chunk = ops.dataset_stage_chunk_bytes()
        self.arena = torch.empty(total, dtype=torch.uint8, pin_memory=True)   # filled in place: the set is never in device memory as a whole
        host = self.arena.numpy()
        for j, im in enumerate(images):
            a, b, c = int(offsets[j]), int(offsets[j]) + im.nbytes, int(offsets[j + 1])
            host[a:b] = im.reshape(-1)
            host[b:c] = 0   # the alignment gap behind the image
        self.src = _upload(rec.view(np.uint8).reshape(-1), device)
        blank = rec.copy()
        blank["offset"] = -1   # not staged: the kernels read such an image as border
        self.ring = torch.empty(2 * self.half_bytes, dtype=torch.uint8, device=device)
        self.halves = [self.ring[: self.half_bytes], self.ring[self.half_bytes :]]
        self.records = [_upload(blank.view(np.uint8).reshape(-1), device) for _ in range(2)]
        self._max_jobs = min(n, int(per_item) * int(batch_size))
        self.pinned = self.dev = None   # reserved once: by the train-mode set for its records, else at the first batch
        self.status = torch.zeros(1, dtype=torch.int32, device=device)
        self.stream = torch.cuda.Stream(device)
        self.stream.wait_stream(torch.cuda.current_stream(device))   # the tables and the status word above were written on the current stream
        self.staged = [torch.cuda.Event() for _ in range(2)]
        self.consumed = [torch.cuda.Event() for _ in range(2)]
        self.last, self.ahead = None, None   # the half of the last batch handed out; (key, half, what `fill` returned) of the batch staged ahead

    def reserve(self, front: int):
        """the pinned buffer of each half and its device twin: `front` bytes for the batch's own records, then the jobs of the largest batch"""
        nbytes = -(-int(front) // 8) * 8 + 24 * self._max_jobs
        self.pinned = [torch.empty(nbytes, dtype=torch.uint8, pin_memory=True) for _ in range(2)]
        self.dev = [torch.empty(nbytes, dtype=torch.uint8, device=self.device) for _ in range(2)]

    def _submit(self, h, needs, fill, stream):
        unique, offsets = plan_slots(needs, self.slots, self.half_bytes)
        if self.pinned is None:
            self.reserve(0)
        self.staged[h].synchronize()   # the pinned buffer of the half is free once the copy of its last batch has run
        pinned, m = self.pinned[h], len(unique)
        end, extra = (0, None) if fill is None else fill(pinned, self.dev[h])   # the batch's own records in front
        at = -(-end // 8) * 8
        if at + 24 * m > pinned.numel():
            raise ValueError(f"HostStore: {m} images in one batch exceed the staging buffer (items drawn for another set?)")
        jobs = stage_jobs(unique, offsets, self.slots, self.chunk)
        pinned.numpy()[at : at + 24 * m].view(np.int64)[:] = jobs.reshape(-1)
        with torch.cuda.stream(stream):
            stream.wait_event(self.consumed[h])
            self.dev[h][: at + 24 * m].copy_(pinned[: at + 24 * m], non_blocking=True)   # the one host -> device copy of the batch: its records and its jobs
            if m:
                ops.dataset_stage(self.arena, self.src, self.n, self.dev[h][at : at + 24 * m].view(torch.int64).view(m, 3), m, int(jobs[-1, 2]), self.halves[h], self.records[h],
                                  self.status)
            self.staged[h].record(stream)
        return extra

    @staticmethod
    def _same(a, b):
        return a is b or (isinstance(a, tuple) and isinstance(b, tuple) and a == b)

    def acquire(self, key, needs, fill=None):
        """-> (half, what `fill` returned): the half staged ahead under `key`, the current stream made to wait for it, else one staged now on the current stream"""
        ahead, self.ahead = self.ahead, None
        if ahead is not None and self._same(ahead[0], key):
            torch.cuda.current_stream(self.device).wait_event(self.staged[ahead[1]])
            self.last = ahead[1]
            return ahead[1], ahead[2]
        self.ahead = ahead   # (a batch out of turn: what was staged ahead keeps its half)
        h = 1 - ahead[1] if ahead is not None else (0 if self.last is None else 1 - self.last)
        extra = self._submit(h, needs, fill, torch.cuda.current_stream(self.device))
        self.last = h
        return h, extra

    def stage_ahead(self, key, needs, fill=None):
        """stage the batch `key` on the side stream into the half the last batch did not use"""
        h = 0 if self.last is None else 1 - self.last
        self.ahead = None
        self.ahead = (key, h, self._submit(h, needs, fill, self.stream))

    def release(self, h):
        """the consumer launches of the half are in the current stream"""
        self.consumed[h].record(torch.cuda.current_stream(self.device))

    def check(self):
        """RuntimeError if the stage skipped a job since the set was built (the kernel's own bound: a plan of this module never trips it)"""
        skipped = int(self.status.item())
        if skipped:
            raise RuntimeError(f"HostStore: y3_dataset_stage skipped {skipped} job(s) that did not fit the host arena or the ring; the batch read border in their place")


class DeviceDataset:
    """The images and labels of a cached augment=False dataset in device memory; iterating yields the reference loader's 4-tuples (im, targets, paths, shapes) with
    `im` (bs, 3, H, W) and `targets` (nl, 6) made on the device, one launch each.

    images   list of (h, w, 3) uint8 BGR arrays as load_image returns them (already resized: the long side <= img_size)
    labels   list of (m, 5) fp32 [cls, x, y, w, h] normalised arrays (what LabelTable takes)
    shapes0  the original (h0, w0) of every image (default: the cached size); rect sorts by their aspect ratio, as the reference sorts by dataset.shapes
    paths    the file name of every image (default: its index as a string)
    rect     True: batches of the aspect-ratio order, each letterboxed to its own shape (rect_batch_shapes).  False: the square img_size, in the given order or
             in the order of set_indices(perm)
    single_cls  zero the class column when the table is built (dataloaders.py:544-545)
    dtype    torch.uint8, or float16 / bfloat16 / float32 for batches already divided by 255
    store    "device" (the default): the whole set in one HBM arena.  "host": the set in pinned host memory, each batch's images staged into an HBM ring of two halves
             (.host_bytes, .ring_bytes; both 0 for a resident set)
    prefetch 1 (the default under store="host"): __iter__ stages batch k + 1 on a side stream before it hands out batch k, so the copy runs under the caller's step; 0: the stage runs inside
             get_batch, on the current stream

    After construction .n, .paths, .shapes, .labels, .batch, .batch_shapes, .top, .left and .order describe the set in ITS order (`order[j]` is the constructor's
    index of image j); len(ds) is the number of batches."""

    def __init__(self, images, labels, img_size=640, batch_size=32, stride=32, pad=0.5, rect=True, shapes0=None, paths=None, single_cls=False, device="cuda",
                 dtype=torch.uint8, _adopt=None, store="device", prefetch=None, _per_item=1):
        # every refusal comes before anything is pinned or uploaded
        prefetch = check_store(type(self).__name__, store, prefetch)
        n = len(images)
        if n < 1:
            raise ValueError("DeviceDataset: no images")
        if len(labels) != n or (shapes0 is not None and len(shapes0) != n) or (paths is not None and len(paths) != n):
            raise ValueError(f"DeviceDataset: {n} images, but {len(labels)} label arrays" + (", or shapes0 / paths of another length" if len(labels) == n else ""))
        if dtype not in _DTYPES:
            raise TypeError(f"DeviceDataset yields uint8 / float16 / bfloat16 / float32 batches, not {dtype}")
        if int(batch_size) < 1 or int(batch_size) > 1024:
            raise ValueError(f"DeviceDataset: batch_size = {batch_size} (1 .. 1024)")
        paths = [str(i) for i in range(n)] if paths is None else [str(p) for p in paths]
        for i, im in enumerate(images):
            if not isinstance(im, np.ndarray) or im.dtype != np.uint8 or im.ndim != 3 or im.shape[2] != 3 or im.shape[0] < 1 or im.shape[1] < 1:
                what = f"{im.dtype} {im.shape}" if isinstance(im, np.ndarray) else type(im).__name__
                raise TypeError(f"DeviceDataset: image {paths[i]} is {what}, not a uint8 (h, w, 3) array")
        table = []
        for i, lb in enumerate(labels):
            lb = np.asarray(lb)
            if lb.ndim != 2 or lb.shape[1] != 5:
                raise ValueError(f"DeviceDataset: the labels of image {paths[i]} have shape {lb.shape}, not (m, 5)")
            lb = lb.astype(np.float32)   # (a copy: single_cls must not reach the caller's arrays)
            if single_cls:
                lb[:, 0] = 0
            table.append(lb)
        hw = [im.shape[:2] for im in images]
        lay = layout(hw, hw if shapes0 is None else shapes0, img_size, batch_size, stride, pad, rect, paths, _adopt)
        device = _device(device)

        self.n, self.img_size, self.batch_size, self.stride, self.pad, self.rect, self.single_cls = n, int(img_size), int(batch_size), int(stride), pad, bool(rect), bool(single_cls)
        self.device, self.dtype = device, dtype
        self.order, self.batch, self.batch_shapes, self.top, self.left, self.shapes = lay
        self.paths = [paths[i] for i in self.order]
        self.labels = [table[i] for i in self.order]
        images = [np.ascontiguousarray(images[i]) for i in self.order]
        rec = np.zeros(n, dtype=_RECORD)
        offsets = np.zeros(n + 1, dtype=np.int64)
        for j, im in enumerate(images):
            offsets[j + 1] = offsets[j] + -(-im.nbytes // _ALIGN) * _ALIGN
            H, W = self.batch_shapes[self.batch[j]]
            rec[j] = (offsets[j], im.shape[0], im.shape[1], self.top[j], self.left[j], H, W)
        self._counts = np.array([len(lb) for lb in self.labels], dtype=np.int64)
        label_offsets = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(self._counts, out=label_offsets[1:])
        self.store, self.prefetch, self._store, self.host_bytes, self.ring_bytes = store, prefetch, None, 0, 0
        if store == "host":   # the arena in pinned host memory and a ring of two halves in HBM; the full-size device arena is never allocated
            self._store = HostStore(images, offsets, rec, _per_item, self.batch_size, device)
            self._arena = self._records = None
            self.host_bytes, self.ring_bytes = self._store.arena.numel(), self._store.ring.numel()
        else:
            self._arena = _upload_arena(images, offsets, int(offsets[-1]), device)
            self._records = _upload(rec.view(np.uint8).reshape(-1), device)
        self._labels = _upload(np.concatenate(self.labels, 0) if label_offsets[-1] else np.zeros((0, 5), dtype=np.float32), device)
        self._label_offsets = _upload(label_offsets, device)
        self._perm, self._perm_dev = None, None

    @classmethod
    def from_dataset(cls, dataset, batch_size, device="cuda", dtype=torch.uint8, single_cls=False, store="device", prefetch=None):
        """From a reference LoadImagesAndLabels built with cache="ram", augment=False: reads .ims, .im_hw0, .im_hw, .labels, .im_files, .rect, .img_size, .stride and,
        where present, .pad, .batch / .batch_shapes (the order the dataset is already in is adopted) and .indices (rect=False: the epoch's order).
        store / prefetch: as for the constructor."""
        ims = list(dataset.ims)
        if any(im is None for im in ims):
            raise ValueError('DeviceDataset.from_dataset: the dataset holds no cached images (build it with cache="ram")')
        if getattr(dataset, "augment", False):
            raise ValueError("DeviceDataset.from_dataset: the dataset augments (augment=True); only the augment=False path is here, DeviceTrainDataset is the train-mode loader")
        for i, (im, hw) in enumerate(zip(ims, dataset.im_hw)):
            if isinstance(im, np.ndarray) and tuple(im.shape[:2]) != tuple(int(v) for v in hw):
                raise ValueError(f"DeviceDataset.from_dataset: im_hw[{i}] = {tuple(hw)} is not the cached image's {im.shape[:2]}")
        rect = bool(dataset.rect)
        adopt = (dataset.batch, dataset.batch_shapes) if rect and hasattr(dataset, "batch") and hasattr(dataset, "batch_shapes") else None
        ds = cls(ims, dataset.labels, img_size=dataset.img_size, batch_size=batch_size, stride=dataset.stride, pad=getattr(dataset, "pad", 0.0), rect=rect,
                 shapes0=[tuple(hw0) for hw0 in dataset.im_hw0], paths=dataset.im_files, single_cls=single_cls, device=device, dtype=dtype, _adopt=adopt, store=store, prefetch=prefetch)
        indices = getattr(dataset, "indices", None)
        if not rect and indices is not None and list(indices) != list(range(ds.n)):
            ds.set_indices(indices)
        return ds

    def set_indices(self, indices):
        """The order of the next epochs (rect=False only): a shuffle or image_weight_indices' draw, a sequence of image indices of any length, uploaded once;
        None restores the set's own order."""
        if self.rect:
            raise ValueError("DeviceDataset.set_indices: a rect=True set keeps its aspect-ratio order (the batch shapes belong to it)")
        if indices is None:
            self._perm, self._perm_dev = None, None
            return
        perm = np.asarray(list(indices))
        if perm.ndim != 1 or len(perm) < 1 or perm.dtype.kind not in "iu" or perm.min() < 0 or perm.max() >= self.n:
            raise ValueError(f"DeviceDataset.set_indices expects image indices in [0, {self.n})")
        self._perm = perm.astype(np.int64)
        self._perm_dev = _upload(self._perm, self.device)

    def __len__(self):
        return math.ceil((self.n if self._perm is None else len(self._perm)) / self.batch_size)

    def batch_images(self, k: int):
        """the images of batch k, in the set's order: a list of indices"""
        total = self.n if self._perm is None else len(self._perm)
        lo, hi = k * self.batch_size, min((k + 1) * self.batch_size, total)
        if not 0 <= lo < hi:
            raise IndexError(f"DeviceDataset: batch {k} of {len(self)}")
        return list(range(lo, hi)) if self._perm is None else self._perm[lo:hi].tolist()

    def get_batch(self, k: int, out: torch.Tensor | None = None):
        """Batch k as the reference loader's 4-tuple (im, targets, paths, shapes); `out`: a tensor to write the images into (ops.dataset_batch)."""
        which = self.batch_images(k)
        count, first = len(which), k * self.batch_size
        idx = None if self._perm is None else self._perm_dev[first : first + count]
        H, W = (int(v) for v in self.batch_shapes[k]) if self.rect else (self.img_size, self.img_size)
        arena, records, half = self._arena, self._records, None
        if self._store is not None:   # the half of the ring that holds the batch's images: staged ahead by __iter__, else staged here on the current stream
            half, _ = self._store.acquire(tuple(which), which)
            arena, records = self._store.halves[half], self._store.records[half]
        try:
            im = ops.dataset_batch(arena, records, self.n, idx, first, count, H, W, self.dtype, out)
            targets, _ = ops.dataset_targets(self._labels, self._label_offsets, records, self.n, idx, first, count, H, W, int(self._counts[which].sum()))
        finally:
            if half is not None:
                self._store.release(half)
        return im, targets, tuple(self.paths[i] for i in which), tuple(self.shapes[i] for i in which)

    def _stage_ahead(self, k: int) -> dict:
        """launch the stage of batch k on the store's side stream -> the keywords get_batch(k) takes to find it"""
        which = self.batch_images(k)
        self._store.stage_ahead(tuple(which), which)
        return {}

    def __iter__(self):
        nb, ahead = len(self), {}
        for k in range(nb):
            batch = self.get_batch(k, **ahead)
            # prefetch: batch k + 1 is drawn and its stage is in the side stream BEFORE batch k is handed out, so the copy runs under whatever the caller does with
            # batch k, a step that ends in a host synchronise included
            ahead = self._stage_ahead(k + 1) if self.prefetch and k + 1 < nb else {}
            yield batch
        if self._store is not None:
            self._store.check()   # (this class reads nothing back per batch: the stage's status word is read once per epoch)
