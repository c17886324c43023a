"""The train-mode loader on the device: mosaic, random affine, HSV, flips and mixup of a cached dataset (reference utils/dataloaders.py:659-735, 764-822;
utils/augmentations.py:57-73, 137-216, 270-283).

    ds = DeviceTrainDataset(images, labels, hyp, img_size=640, batch_size=64)       # or DeviceTrainDataset.from_dataset(train_loader.dataset, batch_size=64)
    ds.set_indices(perm)                                                            # the epoch's order; also the pool load_mosaic's random.choices draws from
    for im, targets, paths, shapes in ds: ...                                       # im (bs, 3, s, s) RGB CHW and targets (nl, 6) are DEVICE tensors

The host keeps the random stream and nothing per pixel: draw_item makes the reference's calls to `random` and `np.random` in the reference's order (a seeded process
stands, after every item, where the reference's __getitem__ would leave both generators) and forms, in float64 and in the reference's operation order, the matrix
M = T @ S @ R @ P @ C, the paste rectangles of load_mosaic, the three HSV look-up tables, the flip flags and the mixup ratio.  They go into one fixed-size record per
item (y3_augment_item); a batch is one pinned host -> device copy of bs records.  csrc/augment.hip does the rest in two launches per batch: y3_augment_batch samples
every output pixel straight from the image arena (the 2s x 2s canvas is never materialised) and y3_augment_targets transforms, filters and compacts the labels.  The
survivor count is known only on the device: the host reads the bs + 1 offsets once per batch.

Polygon labels (segments=..., what the reference's parser makes of label rows with more than six numbers): segments[i] is empty or holds one (k, 2) float32 array of
normalised vertices per label row of image i.  The vertices go up once with the labels, as one fp32 (V, 2) table and one int64 offset per label row plus one
(pack_polygons); per batch one more launch, y3_augment_polygons ahead of the targets, carries every polygon of every mosaic through xyn2xy, the clip, the 1000 samples
of resample_segments, M and segment2box in fp64, and y3_augment_targets_polygons takes those boxes with area_thr 0.01 for a mosaic in which every label row has a
polygon and some clipped coordinate is not zero (random_perspective's use_segments) -- every other mosaic, and every letterbox item, runs the four-corner box path
with 0.10.  Polygons draw no random numbers and touch no pixel.  A set without polygons makes the two launches it always made.

Copy-paste (copy_paste=True; copy_paste(img4, labels4, segments4, p=hyp["copy_paste"]) of load_mosaic, dataloaders.py:809, augmentations.py:219-240): on a set with
polygons draw_mosaic makes random.sample(range(n), k=round(p n)) over the mosaic's polygons at the reference's place, the candidates of a batch go up behind its records
as one int32 table (pack_paste; no new record), and a batch in which some mosaic drew candidates makes five launches (ops.augment_copy_paste): the selection walks the
candidates in order -- box = (w - x2, y1, w - x1, y2) of label row j, accepted when bbox_ioa < 0.30 against every current row; label row j is paired with polygon j of
the list of polygons, as the reference pairs them -- the raster fills the accepted polygons into a 1-bit mask of the canvas, the sampler reads canvas pixel
(w - 1 - x, y) where the mask bit there is set, and the polygon and targets kernels carry the appended rows and mirrored polygons at k reserved positions after the
mosaic's tile rows.  Every other batch -- no candidates, a set without polygons, a letterbox item, copy_paste=False -- makes exactly the launches it made before.

What rests on what: the draws, the geometry, M, the tables, the whole label path, the blend, the flips and the layout are pinned by the unmodified reference
(tests/golden/make_augment_golden.py; the polygon label path by tests/golden/make_augment_polygons_golden.py over label files with polygon rows, through the NumPy
statement of tests/augment_polygon_cases.py, which the generator asserts equal to the reference item by item).  The pixel sampler of cv2.warpAffine and the two
cv2.cvtColor conversions follow the integer / fp32 statements of tests/augment_cases.py, which restate the published 8-bit algorithms and have not been compared with
a cv2 build.  Copy-paste is pinned by the unmodified reference likewise (tests/golden/make_augment_copy_paste_golden.py: the draws, the pairing, the appended rows, the pasted
canvas given the mask, the targets) and rests on two more restatements, tests/augment_copy_paste_cases.py: bbox_ioa of the un-vendored ultralytics package, on which every
acceptance decision rests, and cv2.drawContours(FILLED) (fill_mask), which has not been compared with a cv2 build either: a difference from one, if there is one, lies in
boundary pixels of a paste and never in a label.

Rectangular training (train.py --rect; LoadImagesAndLabels(augment=True, rect=True), dataloaders.py:547-570):

    ds = DeviceRectTrainDataset(images, labels, hyp, img_size=640, batch_size=64, stride=32)   # or DeviceRectTrainDataset.from_dataset(train_loader.dataset, batch_size=64)
    for im, targets, paths, shapes in ds: ...                                                  # im (bs, 3, H_k, W_k): batch k has its own shape

The set is sorted by aspect ratio and laid out as a rect DeviceDataset with pad=0.0 (rect_batch_shapes: every H_k and W_k a multiple of stride, [maxi, 1] for a batch of
wide images, [1, 1 / mini] for one of tall images, else square).  The reference sets mosaic = augment and not rect and forces shuffle off: every item is the letterbox
branch -- pasted at round(dh - 0.1), round(dw - 0.1) on its batch's H x W canvas, random_perspective with C = (-W / 2, -H / 2) and T = (u W, u H), the labels clipped to
[0, W] x [0, H], area_thr 0.10 (segments are accepted and not used, as __getitem__ hands none on), xyxy2xywhn per axis, HSV, the flips; no mixup, and `shapes` is the
letterbox tuple of every item.  draw_item and draw_perspective take the pair (H, W) for this.  The same two launches per batch through y3_augment_batch_hw /
y3_augment_targets_hw: the kernels of csrc/augment.hip work on H x W items, and the square exports call them with H = W = S.  One difference of the reference's own
arithmetic is reproduced: letterbox takes a rect batch's shape from a NumPy array, so its ratio and halves are float64 scalars and NumPy (>= 2) forms xywhn2xyxy's
product and sum in float64 before the fp32 label array rounds them once; the tiles of rect items carry `wide` and the kernel does the same (a square set's labels
stay fp32 throughout, as there).  Pinned by tests/golden/make_augment_rect_golden.py (stride 16, batches of (48, 64), (64, 64) and (64, 48)).

Refused (ValueError) before anything is uploaded: hyp["perspective"] != 0, hyp["copy_paste"] != 0 without copy_paste=True, polygon labels whose count is neither 0 nor the image's label rows
(the reference would send such a mosaic down the box path; here it is an error: a stated difference) or that hold an empty polygon, rect=True on DeviceTrainDataset
(DeviceRectTrainDataset is that loader), an image whose long side is not img_size (load_image's resize is not here), an img_size that is odd or no multiple of 16; on a
rect set an image that letterbox(scaleup=True) would resize (r = min(H / h, W / w) != 1; the message names the image, its size and the batch shape), an img_size or
stride that is no multiple of 16, and set_indices (the batch shapes belong to the order); KeyError for a missing hyp key.  Albumentations is a no-op, as in the
reference when the package is absent.  Out of scope: warpPerspective, a resize inside letterbox, load_mosaic9, cutout, returning the warped polygons.

A set larger than HBM (store="host", both classes and their from_dataset; dataset.HostStore): the images stay in one pinned host tensor and the device holds a ring of
two halves, each sized for the worst batch -- the min(n, t batch_size) largest images, t = 4 for mosaics, 8 when hyp["mixup"] > 0, 1 for a rect set and for mosaic=False --
with its own copy of the record table.  The host knows the images of a batch once its items are drawn (at most 4 per item, 8 with mixup); dataset.plan_slots gives each
unique image a slot in a half, the job table rides up behind the batch's records (and its copy-paste candidates) in the same pinned copy, and ONE launch of
y3_dataset_stage (csrc/dataset_stage.hip) copies those images over PCIe and writes their records with the slots' offsets; the launches above then read (ring half, its
table) where they read (arena, table).  No sampling kernel changes and the batches are bit-identical.  prefetch=1 (the default under store="host"): when __iter__
hands out batch k, the items of batch k + 1 are drawn and their stage is launched on a side stream the set owns, so the copy runs under the caller's step on batch k
whatever that step does; events make the stage wait for the last launches that read the half it overwrites (batch k - 1's) and batch k + 1's launches wait for the
stage.  prefetch=0 draws and stages inside get_batch, on the current stream, exactly where the resident path draws.  get_batch(k) out of turn always works, staging on
the current stream into the half that the batch staged ahead does not occupy.  A stated difference: with prefetch=1 the draws of batch k + 1 are made one batch earlier
in the process's `random` / `np.random` streams, so a caller that draws between batches (multi_scale_size) sees another interleaving than with prefetch=0 -- the
reference's own worker processes fix no such interleaving -- and the batches themselves are unaffected.  The host's draws for batch k + 1 (about 2 ms for 64 mosaics)
stand between batch k and the launch of its step; profiles/dataset_stream_ab.txt has what that costs against a loop whose step ends in a host synchronise and one
whose step does not.  Refused
(ValueError) before anything is pinned or uploaded: an unknown store, prefetch not in (0, 1), prefetch=1 with store="device".  .host_bytes and .ring_bytes tell what the
set takes on either side (0 for a resident set).  The stage's status word (jobs the kernel skipped because they did not fit: none for a plan of this module) is read
right after the batch's offsets; RuntimeError if it is not zero.
"""
from __future__ import annotations

import math
import random
from dataclasses import dataclass

import numpy as np
import torch

from . import ops
from . import dataset as _dataset
from .dataset import DeviceDataset

HYP_KEYS = ("mosaic", "mixup", "degrees", "translate", "scale", "shear", "perspective", "hsv_h", "hsv_s", "hsv_v", "flipud", "fliplr", "copy_paste")

# y3_augment_tile / y3_augment_mosaic / y3_augment_item as include/yolov3_hip.h declares them
TILE, MOSAIC, ITEM = np.dtype(ops.Y3AugmentTile), np.dtype(ops.Y3AugmentMosaic), np.dtype(ops.Y3AugmentItem)
assert (TILE.itemsize, MOSAIC.itemsize, ITEM.itemsize) == (40, 280, 1360)


@dataclass
class Mosaic:
    """One canvas and its warp: `indices` the images of the tiles in paste order, `rects` per tile (x1a, y1a, x2a, y2a, x1b, y1b, x2b, y2b), `M` the 3 x 3 float64
    matrix of random_perspective, `scale` its s, `canvas` the side of the canvas (2 s, or s for the letterbox branch), `pad` per tile the (padw, padh) of its labels;
    `canvas_h` the height of the canvas of a rect item (`canvas` is then its width; the labels of such an item go through xywhn2xyxy in float64), else None."""

    indices: list
    rects: list
    M: np.ndarray
    scale: float
    canvas: int
    pad: list
    center: tuple | None = None   # (yc, xc)
    canvas_h: int | None = None
    paste: tuple = ()             # copy_paste's js: random.sample over the polygons of the mosaic, in the order drawn


@dataclass
class Item:
    index: int
    mosaics: list
    ratio: float | None       # the mixup ratio r, or None
    luts: np.ndarray | None   # (3, 256) uint8: hue, sat, val; None when every gain is 0
    flipud: bool
    fliplr: bool
    mosaic: bool              # False: the letterbox branch (one tile on an s x s canvas)


def rotation_matrix_2d(angle, scale):
    """cv2.getRotationMatrix2D(center=(0, 0)) from its documented formula -> the two rows"""
    a = angle * math.pi / 180
    alpha, beta = math.cos(a) * scale, math.sin(a) * scale
    return [[alpha, beta, (1 - alpha) * 0 - beta * 0], [-beta, alpha, beta * 0 + (1 - alpha) * 0]]


def _hw(size):
    """img_size, or the (H, W) of a rect batch -> (H, W)"""
    return (int(size[0]), int(size[1])) if isinstance(size, (tuple, list, np.ndarray)) else (int(size), int(size))


def draw_perspective(hyp, side, border):
    """random_perspective's eight draws and its matrix for a (side, side) image, or the (H, W) image `side` names as a pair: -> (M (3, 3) float64, s)"""
    h, w = side if isinstance(side, (tuple, list, np.ndarray)) else (side, side)
    height, width = h + border * 2, w + border * 2
    C, P, R, S, T = (np.eye(3) for _ in range(5))
    C[0, 2] = -w / 2
    C[1, 2] = -h / 2
    perspective = hyp["perspective"]
    P[2, 0] = random.uniform(-perspective, perspective)
    P[2, 1] = random.uniform(-perspective, perspective)
    a = random.uniform(-hyp["degrees"], hyp["degrees"])
    s = random.uniform(1 - hyp["scale"], 1 + hyp["scale"])
    R[:2] = rotation_matrix_2d(a, s)
    S[0, 1] = math.tan(random.uniform(-hyp["shear"], hyp["shear"]) * math.pi / 180)
    S[1, 0] = math.tan(random.uniform(-hyp["shear"], hyp["shear"]) * math.pi / 180)
    T[0, 2] = random.uniform(0.5 - hyp["translate"], 0.5 + hyp["translate"]) * width
    T[1, 2] = random.uniform(0.5 - hyp["translate"], 0.5 + hyp["translate"]) * height
    return T @ S @ R @ P @ C, s   # (NumPy's matrix product, as the reference forms it)


def draw_mosaic(index, hw, hyp, s, pool, poly_counts=None) -> Mosaic:
    """load_mosaic's draws and geometry (dataloaders.py:764-822).  poly_counts: the number of polygons of every image, for copy_paste's draw (augmentations.py:223-227:
    n = len(segments4), nothing unless p and n, else random.sample(range(n), k=round(p * n)), between the shuffle and random_perspective's uniforms); None: no draw."""
    border = -s // 2
    yc, xc = (int(random.uniform(-x, 2 * s + x)) for x in (border, border))
    indices = [index, *random.choices(pool, k=3)]
    random.shuffle(indices)
    rects, pad = [], []
    for i, j in enumerate(indices):
        h, w = hw[j]
        if i == 0:
            x1a, y1a, x2a, y2a = max(xc - w, 0), max(yc - h, 0), xc, yc
            x1b, y1b, x2b, y2b = w - (x2a - x1a), h - (y2a - y1a), w, h
        elif i == 1:
            x1a, y1a, x2a, y2a = xc, max(yc - h, 0), min(xc + w, s * 2), yc
            x1b, y1b, x2b, y2b = 0, h - (y2a - y1a), min(w, x2a - x1a), h
        elif i == 2:
            x1a, y1a, x2a, y2a = max(xc - w, 0), yc, xc, min(s * 2, yc + h)
            x1b, y1b, x2b, y2b = w - (x2a - x1a), 0, w, min(y2a - y1a, h)
        else:
            x1a, y1a, x2a, y2a = xc, yc, min(xc + w, s * 2), min(s * 2, yc + h)
            x1b, y1b, x2b, y2b = 0, 0, min(w, x2a - x1a), min(y2a - y1a, h)
        rects.append((x1a, y1a, x2a, y2a, x1b, y1b, x2b, y2b))
        pad.append((x1a - x1b, y1a - y1b))
    paste = ()
    if poly_counts is not None:
        p, n = hyp["copy_paste"], sum(int(poly_counts[j]) for j in indices)
        if p and n:
            paste = tuple(random.sample(range(n), k=round(p * n)))
    M, scale = draw_perspective(hyp, 2 * s, border)
    return Mosaic([int(j) for j in indices], rects, M, scale, 2 * s, pad, (yc, xc), None, paste)


def draw_item(index, hw, hyp, img_size, pool=None, n=None, mosaic=True, poly_counts=None) -> Item:
    """The draws of one __getitem__ (dataloaders.py:659-735) for image `index` (already looked up in the epoch's order), from the global `random` and `np.random`, in
    the reference's order: random.random() for mosaic; load_mosaic (two uniforms, yc then xc, choices(pool, k=3), shuffle) and random_perspective's eight uniforms;
    random.random() for mixup and, on mixup, randint(0, n - 1), a second load_mosaic and np.random.beta(32, 32) -- or the letterbox branch with its one
    random_perspective; np.random.uniform(-1, 1, 3) if an HSV gain is non-zero; random.random() for flipud, then for fliplr.
    hw: the cached (h, w) of every image; pool: the epoch's order (default range(n)); n: the number of images (default len(hw)).
    img_size: the side of the square item, or the (H, W) of a rect batch, whose items are drawn with mosaic=False (the reference's mosaic = augment and not rect).
    The shape of a rect batch is an element of a NumPy array in the reference, so letterbox's ratio and halves are float64 scalars there and NumPy (>= 2) forms
    xywhn2xyxy's product and sum in float64 before the label array rounds them: such an item's Mosaic carries canvas_h, and the kernel does the same.
    poly_counts: per image its number of polygons, for a set built with copy_paste=True: every load_mosaic then makes copy_paste's random.sample (draw_mosaic)."""
    H, W = _hw(img_size)
    rect = isinstance(img_size, (tuple, list, np.ndarray))   # the batch shape of a rect set, a square one included
    if mosaic and H != W:
        raise ValueError(f"draw_item: a {H}x{W} item is a rect batch's; load_mosaic is square (mosaic=False)")
    s = W
    n = len(hw) if n is None else int(n)
    pool = range(n) if pool is None else pool
    ratio = None
    if mosaic and random.random() < hyp["mosaic"]:
        is_mosaic = True
        mosaics = [draw_mosaic(index, hw, hyp, s, pool, poly_counts)]
        if random.random() < hyp["mixup"]:
            mosaics.append(draw_mosaic(random.randint(0, n - 1), hw, hyp, s, pool, poly_counts))
            ratio = float(np.random.beta(32.0, 32.0))
    else:
        is_mosaic = False
        h, w = hw[index]
        dw, dh = (W - w) / 2, (H - h) / 2
        top, left = round(dh - 0.1), round(dw - 0.1)
        M, scale = draw_perspective(hyp, (H, W) if rect else s, 0)
        mosaics = [Mosaic([int(index)], [(left, top, left + w, top + h, 0, 0, w, h)], M, scale, s, [(dw, dh)], None, H if rect else None)]
    luts = None
    if hyp["hsv_h"] or hyp["hsv_s"] or hyp["hsv_v"]:
        r = np.random.uniform(-1, 1, 3) * [hyp["hsv_h"], hyp["hsv_s"], hyp["hsv_v"]] + 1
        x = np.arange(0, 256, dtype=r.dtype)
        luts = np.stack([((x * r[0]) % 180).astype(np.uint8), np.clip(x * r[1], 0, 255).astype(np.uint8), np.clip(x * r[2], 0, 255).astype(np.uint8)])
    flipud = random.random() < hyp["flipud"]
    fliplr = random.random() < hyp["fliplr"]
    return Item(int(index), mosaics, ratio, luts, bool(flipud), bool(fliplr), is_mosaic)


def invert_affine(M):
    """cv2.invertAffineTransform of the first two rows, float64 -> (A00, A01, A02, A10, A11, A12)"""
    m00, m01, m02, m10, m11, m12 = (float(v) for v in np.asarray(M, dtype=np.float64)[:2].reshape(-1))
    D = m00 * m11 - m01 * m10
    D = 1.0 / D if D != 0 else 0.0
    a00, a11 = m11 * D, m00 * D
    a01, a10 = m01 * -D, m10 * -D
    return a00, a01, -a00 * m02 - a01 * m12, a10, a11, -a10 * m02 - a11 * m12


def pack_items(items, out=None) -> np.ndarray:
    """the records of a batch: a structured array of ITEM (1360 bytes each), written into `out` when given"""
    rec = np.zeros(len(items), dtype=ITEM) if out is None else out
    rec[...] = np.zeros((), dtype=ITEM)
    for b, it in enumerate(items):
        r = rec[b]
        r["nmos"], r["flipud"], r["fliplr"], r["hsv"] = len(it.mosaics), int(it.flipud), int(it.fliplr), int(it.luts is not None)
        if it.ratio is not None:
            r["ratio"], r["ratio1"] = it.ratio, 1 - it.ratio
        if it.luts is not None:
            r["lut"] = it.luts
        for k, mo in enumerate(it.mosaics):
            m = r["mosaics"][k]
            m["inv"], m["m"], m["scale"] = invert_affine(mo.M), mo.M[:2].reshape(-1), mo.scale
            m["ntiles"], m["canvas"], m["clip"] = len(mo.indices), mo.canvas, int(it.mosaic)
            m["canvas_h"] = 0 if mo.canvas_h is None else mo.canvas_h
            for t, (j, rect, (padw, padh)) in enumerate(zip(mo.indices, mo.rects, mo.pad)):
                x1a, y1a, x2a, y2a, x1b, y1b = rect[:6]
                m["tiles"][t] = (j, x1a, y1a, x2a, y2a, x1a - x1b, y1a - y1b, padw, padh, int(mo.canvas_h is not None))
    return rec


def pack_paste(items):
    """The copy-paste candidates of a batch as the device reads them -> (table int32 (4 count + 1 + nk,), nk, masks): 2 count + 1 offsets into the candidates per
    (item, mosaic), 2 count mask indices (the mosaics with candidates numbered in order, -1 for the others), then the js of all mosaics back to back; nk their number,
    masks the number of mosaics with candidates.  No new record: y3_augment_item keeps its 1360 bytes."""
    count = len(items)
    ks = [len(it.mosaics[m].paste) if m < len(it.mosaics) and it.mosaic else 0 for it in items for m in range(2)]
    table = np.zeros(4 * count + 1 + sum(ks), dtype=np.int32)
    np.cumsum(ks, out=table[1 : 2 * count + 1])
    has = np.array(ks) > 0
    table[2 * count + 1 : 4 * count + 1] = np.where(has, np.cumsum(has) - 1, -1)
    table[4 * count + 1 :] = [j for it in items if it.mosaic for mo in it.mosaics for j in mo.paste]
    return table, int(sum(ks)), int(has.sum())


def pack_polygons(labels, segments, paths=None):
    """The polygons of a set as the device reads them -> (vertices (V, 2) float32, offsets (rows + 1,) int64): the vertices of every polygon back to back in the order of
    the label table, row r of the table owning vertices[offsets[r] : offsets[r + 1]]; the rows of an image without polygons own nothing.  segments[i] is empty or holds
    one (k, 2) array, k >= 1, per label row of image i (what the reference's parser and its filters keep): ValueError for any other count and for an empty polygon
    (np.interp raises on one)."""
    if len(segments) != len(labels):
        raise ValueError(f"DeviceTrainDataset: polygon labels for {len(segments)} images, but {len(labels)} label arrays")
    verts, counts = [], []
    for i, (lb, sg) in enumerate(zip(labels, segments)):
        name = paths[i] if paths is not None else i
        if len(sg) == 0:
            counts.extend([0] * len(lb))
            continue
        if len(sg) != len(lb):
            raise ValueError(f"DeviceTrainDataset: image {name} holds {len(sg)} polygon labels for {len(lb)} label rows; segments[i] is empty or has one polygon per row")
        for p in sg:
            p = np.asarray(p)
            if p.ndim != 2 or p.shape[1] != 2 or len(p) < 1:
                raise ValueError(f"DeviceTrainDataset: image {name}: a polygon of its polygon labels has shape {p.shape}, not (k, 2) with k >= 1")
            verts.append(p.astype(np.float32))
            counts.append(len(p))
    offsets = np.zeros(len(counts) + 1, dtype=np.int64)
    np.cumsum(counts, out=offsets[1:])
    vertices = np.concatenate(verts, 0) if verts else np.zeros((0, 2), dtype=np.float32)
    if (np.diff(offsets) < 0).any() or offsets[0] != 0 or offsets[-1] != len(vertices) or len(vertices) > 0x3FFFFFFF:
        raise ValueError(f"DeviceTrainDataset: the polygon labels do not pack ({len(vertices)} vertices, offsets ending at {offsets[-1]})")
    return np.ascontiguousarray(vertices), offsets


class _DeviceAugmentDataset(DeviceDataset):
    """What the two train-mode datasets share; every message names the class the caller used."""

    @classmethod
    def _read_hyp(cls, hyp, copy_paste):
        hyp = {k: hyp[k] for k in HYP_KEYS}   # KeyError for a key the path reads and does not find
        if hyp["perspective"] != 0:
            raise ValueError(f"{cls.__name__}: hyp['perspective'] = {hyp['perspective']}; warpPerspective is not built")
        if hyp["copy_paste"] != 0 and not copy_paste:
            raise ValueError(f"{cls.__name__}: hyp['copy_paste'] = {hyp['copy_paste']}; copy-paste is not built")
        return hyp

    @classmethod
    def _cached(cls, dataset, batch_size, device, dtype, single_cls, copy_paste, store="device", prefetch=None):
        """from_dataset's shared refusals -> (the cached images, the constructor arguments both classes read from the dataset)"""
        ims = list(dataset.ims)
        if any(im is None for im in ims):
            raise ValueError(f'{cls.__name__}.from_dataset: the dataset holds no cached images (build it with cache="ram")')
        if not getattr(dataset, "augment", False):
            raise ValueError(f"{cls.__name__}.from_dataset: the dataset does not augment (augment=False); use DeviceDataset")
        return ims, dict(img_size=dataset.img_size, batch_size=batch_size, stride=dataset.stride, shapes0=[tuple(hw0) for hw0 in dataset.im_hw0], paths=dataset.im_files,
                         single_cls=single_cls, device=device, dtype=dtype, segments=getattr(dataset, "segments", None), copy_paste=copy_paste, store=store, prefetch=prefetch)

    def _set_up(self, hyp, images, mosaic=False, poly_counts=None):
        """what draw_batch reads, and the pinned records of one batch with their device twin; the copy-paste candidates of a batch ride behind its records"""
        self.hyp, self.mosaic, self._poly_counts = hyp, bool(mosaic), poly_counts
        self.hw = [tuple(int(v) for v in images[i].shape[:2]) for i in self.order]   # in the set's order, as the record table is
        nbytes = self.batch_size * ITEM.itemsize
        room = 0 if poly_counts is None else 4 * (4 * self.batch_size + 1 + 8 * self.batch_size * max(poly_counts))
        self._room = nbytes + room
        if self._store is not None:   # store="host": each half of the ring has its own pinned records and device twin, the stage's jobs behind them
            self._store.reserve(self._room)
            return
        self._stage = torch.empty(nbytes + room, dtype=torch.uint8).pin_memory()
        self._stage_rec = self._stage.numpy()[:nbytes].view(ITEM)
        self._items_dev = torch.empty(nbytes + room, dtype=torch.uint8, device=self.device)

    def _pack(self, items, stage, items_dev):
        """Pack the records of the batch, and behind them the int32 table of `_paste`, into the pinned `stage` -> (the bytes packed, None or (the table's place in
        `items_dev`, its candidates, its mosaics with candidates)): what travels with a staged batch, so the launches pair the table with the counts it was made with."""
        paste = self._paste(items)
        nbytes = end = len(items) * ITEM.itemsize
        if paste is not None:
            end = nbytes + paste[0].nbytes
        if end > self._room:
            raise ValueError(f"{type(self).__name__}: {0 if paste is None else paste[0].size - 4 * len(items) - 1} copy-paste candidates in one batch exceed the staging buffer (items drawn for another set?)")
        pack_items(items, stage.numpy()[:nbytes].view(ITEM))
        if paste is None:
            return end, None
        stage.numpy()[nbytes:end].view(np.int32)[:] = paste[0]
        return end, (items_dev[nbytes:end].view(torch.int32), paste[1], paste[2])

    def _upload_items(self, items):
        """pack the records of the batch and the table behind them and make the one host -> device copy of the batch -> what _pack returns second"""
        end, paste = self._pack(items, self._stage, self._items_dev)
        self._items_dev[:end].copy_(self._stage[:end], non_blocking=True)
        return paste

    def _paste(self, items):
        """(the int32 table that rides behind the records of the batch, its candidates, its mosaics with candidates) or None: pack_paste for a DeviceTrainDataset batch that pastes"""
        return None

    @staticmethod
    def _needs(items):
        """the images the launches of the batch read: every tile of every mosaic, at most 4 per item, or 8 with mixup"""
        return [j for it in items for mo in it.mosaics for j in mo.indices]

    def _source(self, items):
        """What the launches of the batch read -> (arena, record table, item records, what _pack returns second, the half of the ring or None).  A resident set:
        its arena and table, after the batch's one host -> device copy.  store="host": a half of the ring with its own table -- the one staged ahead for these
        `items`, else staged now on the current stream; the records of the batch went up in the same pinned copy as the stage's jobs."""
        if self._store is None:
            return self._arena, self._records, self._items_dev, self._upload_items(items), None
        st = self._store
        half, paste = st.acquire(items, self._needs(items), lambda stage, dev: self._pack(items, stage, dev))
        return st.halves[half], st.records[half], st.dev[half], paste, half

    def _stage_ahead(self, k: int) -> dict:
        """draw the items of batch k now and launch their stage on the store's side stream -> the keywords get_batch(k) takes"""
        items = self.draw_batch(k)
        self._store.stage_ahead(items, self._needs(items), lambda stage, dev: self._pack(items, stage, dev))
        return {"items": items}

    def draw_batch(self, k: int):
        """the items of batch k, drawn now from the global generators: a list of Item (a rect set draws every item for its batch's shape, without a mosaic)"""
        pool = range(self.n) if self._perm is None else self._perm.tolist()
        size = tuple(int(v) for v in self.batch_shapes[k]) if self.rect else self.img_size
        return [draw_item(i, self.hw, self.hyp, size, pool, self.n, self.mosaic, self._poly_counts) for i in self.batch_images(k)]

    def get_batch(self, k: int, out: torch.Tensor | None = None, items=None):
        """Batch k as the reference loader's 4-tuple; `items`: what draw_batch returned for it (default: drawn here)."""
        items = self.draw_batch(k) if items is None else items
        im, targets, offsets = self._launch(k, items, out)   # the upload (store="host": the stage, unless it ran ahead), then the launches of the class
        nl = int(offsets.cpu()[len(items)])   # the survivors are counted on the device: the one device -> host read (it also frees the staging buffer for the next batch)
        if self._store is not None:
            self._store.check()   # the stage's status word, read where the batch is read
        return im, targets[:nl], tuple(self.paths[it.index] for it in items), tuple(None if it.mosaic else self.shapes[it.index] for it in items)


class DeviceTrainDataset(_DeviceAugmentDataset):
    """The cached images and labels of an augment=True, rect=False dataset in device memory (the arena, the record table, the label table and the chunked upload of
    DeviceDataset); iterating yields the reference loader's 4-tuples with mosaic, random_perspective (affine), augment_hsv, the flips and mixup applied on the
    device.  shapes[i] is None for a mosaic item, the letterbox tuple otherwise.  hyp: the reference's hyperparameter dict (HYP_KEYS are read).  segments: the
    reference's dataset.segments (per image an empty list, or one (k, 2) float32 polygon per label row); after a batch of a set with polygons `.polygons` holds the
    (boxes, inside, path words) ops.augment_polygons wrote for it.
    copy_paste: False (the default) refuses a non-zero hyp["copy_paste"] as before -- the default is what it is because existing tests pin that refusal and its text;
    a later change may flip it.  True accepts it: on a set with polygons every load_mosaic draws and pastes as the reference's copy_paste does (`.pastes` holds the
    selection tables and the masks of the last batch that pasted, else None); a set without polygons and a letterbox item never paste, as in the reference.
    store / prefetch: "host" keeps the images in pinned host memory and stages each batch's into an HBM ring, by default one batch ahead on a side stream (the module docstring);
    the default "device" is the resident set."""

    def __init__(self, images, labels, hyp, img_size=640, batch_size=64, stride=32, shapes0=None, paths=None, single_cls=False, mosaic=True, device="cuda", dtype=torch.uint8,
                 rect=False, segments=None, copy_paste=False, store="device", prefetch=None):
        # every refusal comes before anything is uploaded
        _dataset.check_store("DeviceTrainDataset", store, prefetch)
        hyp = self._read_hyp(hyp, copy_paste)
        polygons = None
        if segments is not None and any(len(sg) for sg in segments):
            polygons = pack_polygons(labels, segments, paths)   # (host only: the vertex table goes up after the images)
        if rect:
            raise ValueError("DeviceTrainDataset: rect=True; the reference sets mosaic = augment and not rect, use DeviceRectTrainDataset for augmented rectangular batches "
                             "(DeviceDataset for augment=False)")
        if int(img_size) != img_size or int(img_size) < 16 or int(img_size) % 16:
            raise ValueError(f"DeviceTrainDataset: img_size = {img_size} must be a multiple of 16 (hence even: the mosaic border is img_size / 2)")
        for i, im in enumerate(images):
            if isinstance(im, np.ndarray) and im.ndim == 3 and max(im.shape[:2]) != int(img_size):
                raise ValueError(f"DeviceTrainDataset: image {paths[i] if paths is not None else i} is {im.shape[0]}x{im.shape[1]}: its long side is not img_size = "
                                 f"{img_size} (load_image's cv2.resize is out of scope)")
        super().__init__(images, labels, img_size=img_size, batch_size=batch_size, stride=stride, pad=0.0, rect=False, shapes0=shapes0, paths=paths, single_cls=single_cls,
                         device=device, dtype=dtype, store=store, prefetch=prefetch, _per_item=((8 if hyp["mixup"] > 0 else 4) if mosaic else 1))
        self._vertices = self._vertex_offsets = self.polygons = self.pastes = None   # a box-only set: the two launches per batch and nothing else
        if polygons is not None:
            self._vertices, self._vertex_offsets = _dataset._upload(polygons[0], self.device), _dataset._upload(polygons[1], self.device)
        pasting = polygons is not None and copy_paste and hyp["copy_paste"]   # copy_paste's draw per load_mosaic, from the polygon count of every image
        self._set_up(hyp, images, mosaic, [len(sg) for sg in segments] if pasting else None)

    @classmethod
    def from_dataset(cls, dataset, batch_size, device="cuda", dtype=torch.uint8, single_cls=False, copy_paste=False, store="device", prefetch=None):
        """From a reference LoadImagesAndLabels built with cache="ram", augment=True, rect=False: reads .ims, .im_hw0, .im_hw, .labels, .segments, .im_files, .hyp,
        .img_size, .stride, .rect, .mosaic and .indices (the epoch's order).  copy_paste, store, prefetch: as for the constructor."""
        ims, shared = cls._cached(dataset, batch_size, device, dtype, single_cls, copy_paste, store, prefetch)
        ds = cls(ims, dataset.labels, dataset.hyp, mosaic=getattr(dataset, "mosaic", True), rect=bool(dataset.rect), **shared)
        indices = getattr(dataset, "indices", None)
        if indices is not None and list(indices) != list(range(ds.n)):
            ds.set_indices(indices)
        return ds

    def _launch(self, k, items, out):
        upper = int(sum(self._counts[j] for it in items for mo in it.mosaics for j in mo.indices))
        arena, records, items_dev, paste, half = self._source(items)
        batch = (records, self.n, items_dev, len(items), self.img_size)
        try:
            if paste is not None:   # some mosaic pastes: the five launches of the copy-paste form
                table, nk, masks = paste
                im, targets, offsets, self.polygons, self.pastes = ops.augment_copy_paste(self._labels, self._label_offsets, self._vertices, self._vertex_offsets, arena, *batch,
                                                                                          upper + nk, table, nk, masks, self.dtype, out)
                return im, targets, offsets
            self.pastes = None
            im = ops.augment_batch(arena, *batch, self.dtype, out)
            if self._vertices is None:
                return (im, *ops.augment_targets(self._labels, self._label_offsets, *batch, upper))
            # polygon labels: the boxes of the warped polygons first, then the targets that choose per mosaic between them and the four corners
            self.polygons = ops.augment_polygons(self._vertices, self._vertex_offsets, self._label_offsets, *batch, upper)
            return (im, *ops.augment_targets_polygons(self._labels, self._label_offsets, *batch, upper, *self.polygons))
        finally:
            if half is not None:
                self._store.release(half)

    def _paste(self, items):
        if self._poly_counts is not None and any(mo.paste for it in items if it.mosaic for mo in it.mosaics):
            return pack_paste(items)
        return None


class DeviceRectTrainDataset(_DeviceAugmentDataset):
    """The cached images and labels of an augment=True, rect=True dataset in device memory (train.py --rect): the set sorted by aspect ratio and every batch k
    letterboxed to its own batch_shapes[k] = (H_k, W_k), as a rect DeviceDataset with pad=0.0 lays it out; no mosaic and no mixup, every item the letterbox branch
    with random_perspective (affine), augment_hsv and the flips on the device.  Iterating yields (im (bs, 3, H_k, W_k), targets (nl, 6), paths, shapes), shapes[i] the
    letterbox tuple of every item.  hyp: the reference's dict (HYP_KEYS are read; `mosaic` and `mixup` are not used).  segments: accepted and not used, as the
    reference hands none to random_perspective on this branch (area_thr stays 0.10).  The order is the set's: set_indices raises.
    copy_paste: False (the default) refuses a non-zero hyp["copy_paste"] as before (existing tests pin it; a later change may flip it); True accepts the hyp and
    ignores it: the reference's rect path never calls copy_paste.
    store / prefetch: as for DeviceTrainDataset; a rect item reads one image, so a ring half holds the batch_size largest."""

    def __init__(self, images, labels, hyp, img_size=640, batch_size=64, stride=32, shapes0=None, paths=None, single_cls=False, device="cuda", dtype=torch.uint8,
                 segments=None, _adopt=None, copy_paste=False, store="device", prefetch=None):
        # every refusal comes before anything is uploaded
        _dataset.check_store("DeviceRectTrainDataset", store, prefetch)
        hyp = self._read_hyp(hyp, copy_paste)
        for name, v in (("img_size", img_size), ("stride", stride)):
            if int(v) != v or int(v) < 16 or int(v) % 16:
                raise ValueError(f"DeviceRectTrainDataset: {name} = {v} must be a multiple of 16 (both sides of every batch shape are multiples of stride)")
        if all(isinstance(im, np.ndarray) and im.ndim == 3 for im in images) and (shapes0 is None or len(shapes0) == len(images)):   # (else the shared constructor refuses)
            self._refuse_resize(images, [im.shape[:2] for im in images] if shapes0 is None else shapes0, int(img_size), int(batch_size), int(stride), paths, _adopt)
        super().__init__(images, labels, img_size=img_size, batch_size=batch_size, stride=stride, pad=0.0, rect=True, shapes0=shapes0, paths=paths, single_cls=single_cls,
                         device=device, dtype=dtype, _adopt=_adopt, store=store, prefetch=prefetch)
        self._set_up(hyp, images)

    @staticmethod
    def _refuse_resize(images, hw0, img_size, batch_size, stride, paths, adopt):
        """letterbox(scaleup=True) resizes unless r = min(H / h, W / w) is exactly 1: ValueError for the first image of the set's order for which it is not"""
        n = len(images)
        if n < 1 or int(batch_size) < 1:
            return   # (the shared constructor refuses these)
        if adopt is not None:
            order, batch, batch_shapes = np.arange(n), np.asarray(adopt[0]).astype(int), np.asarray(adopt[1]).astype(int).reshape(-1, 2)
            if len(batch) != n or batch.min() < 0 or batch.max() >= len(batch_shapes):
                return   # (layout refuses a batch index that was not built for this set)
        else:
            order, batch, batch_shapes = _dataset.rect_batch_shapes([(w0, h0) for h0, w0 in hw0], img_size, batch_size, stride, 0.0)
        for j, i in enumerate(order):
            (h, w), (H, W) = images[i].shape[:2], (int(v) for v in batch_shapes[batch[j]])
            if h < 1 or w < 1 or min(H / h, W / w) != 1.0:
                raise ValueError(f"DeviceRectTrainDataset: image {paths[i] if paths is not None else i} is {h}x{w} and its batch shape {H}x{W}: letterbox(scaleup=True) "
                                 "would resize it (r != 1), and cv2.resize is out of scope")

    @classmethod
    def from_dataset(cls, dataset, batch_size, device="cuda", dtype=torch.uint8, single_cls=False, copy_paste=False, store="device", prefetch=None):
        """From a reference LoadImagesAndLabels built with cache="ram", augment=True, rect=True: reads .ims, .im_hw0, .im_hw, .labels, .im_files, .hyp, .img_size,
        .stride, .rect, .augment and, where present, .segments and .batch / .batch_shapes (the aspect-ratio order the dataset is already in is adopted).
        copy_paste: as for the constructor (True accepts a non-zero hyp["copy_paste"] and ignores it); store, prefetch: as for the constructor."""
        ims, shared = cls._cached(dataset, batch_size, device, dtype, single_cls, copy_paste, store, prefetch)
        if not dataset.rect:
            raise ValueError("DeviceRectTrainDataset.from_dataset: the dataset is not rectangular (rect=False); use DeviceTrainDataset")
        for i, (im, hw) in enumerate(zip(ims, dataset.im_hw)):
            if isinstance(im, np.ndarray) and tuple(im.shape[:2]) != tuple(int(v) for v in hw):
                raise ValueError(f"DeviceRectTrainDataset.from_dataset: im_hw[{i}] = {tuple(hw)} is not the cached image's {im.shape[:2]}")
        adopt = (dataset.batch, dataset.batch_shapes) if hasattr(dataset, "batch") and hasattr(dataset, "batch_shapes") else None
        return cls(ims, dataset.labels, dataset.hyp, _adopt=adopt, **shared)

    def _launch(self, k, items, out):
        arena, records, items_dev, _, half = self._source(items)
        batch = (records, self.n, items_dev, len(items), *(int(v) for v in self.batch_shapes[k]))
        try:
            im = ops.augment_batch_hw(arena, *batch, self.dtype, out)
            return (im, *ops.augment_targets_hw(self._labels, self._label_offsets, *batch, int(sum(self._counts[it.index] for it in items))))
        finally:
            if half is not None:
                self._store.release(half)
