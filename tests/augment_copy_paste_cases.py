"""Shared inputs of the copy-paste tests of the train-mode dataset (tests/test_augment_copy_paste_cpu.py, tests/test_gpu_augment_copy_paste.py,
tests/golden/make_augment_copy_paste_golden.py): the cases, and the NumPy statement of copy_paste (reference utils/augmentations.py:219-240) inside load_mosaic as
csrc/augment.hip computes it.  Not a test file.

Two definitions live outside the reference tree and are written here once:

  * bbox_ioa of the un-vendored ultralytics package, by its published definition: per axis (min of the upper ends - max of the lower ends).clip(0), the product
    divided by area(box2) + 1e-7, everything fp32 as NumPy >= 2 types it.  The acceptance decisions of every paste rest on this restatement.
  * cv2.drawContours(thickness=FILLED) for an 8-bit image, shift = 0, line_type = 8, by OpenCV's published algorithm: the closed boundary as 8-connected lines between
    the truncated vertices (clipLine to the canvas, then LineIterator's integer stepping from the end with the smaller x), the interior by scan lines over the
    non-horizontal edges, y0 <= y < y1, the edge x in 16.16 fixed point with dx = trunc(((xb - xa) << 16) / (yb - ya)), the crossings of a line sorted and paired,
    a span from (x_left + 65535) >> 16 to x_right >> 16, everything clipped to the canvas (a vertex at 2 S lies outside it).

NEITHER HAS BEEN COMPARED WITH A cv2 / ultralytics BUILD (none is on the build machine); csrc/augment.hip must match fill_mask bit for bit.  A difference from a cv2
build, if there is one, lies in boundary pixels of a paste and never in a label.
"""
from __future__ import annotations

import zlib

import numpy as np

import augment_cases as ac
import augment_polygon_cases as apc

IMG_SIZE, STRIDE, BATCH = ac.IMG_SIZE, ac.STRIDE, ac.BATCH
PROBABILITIES = (0.1, 0.5, 1.0)
SEEDS = {"exact": 0, "low": 0, "wild": 0}   # from the generator's --search: every situation of its check_situations occurs


def cases() -> dict:
    """`exact`, `low` and `wild` of augment_polygon_cases.CASES, each with copy_paste 0.1, 0.5 and 1.0: name -> dict(hyp, seed, indices, base)"""
    out = {}
    for base in ("exact", "low", "wild"):
        for p in PROBABILITIES:
            c = apc.CASES[base]
            out[f"{base}_{p}"] = dict(hyp=dict(c["hyp"], copy_paste=p), seed=SEEDS[base], indices=c["indices"], base=base)
    return out


# ---- bbox_ioa -----------------------------------------------------------------------------------------------------------------------------------------------------------
def bbox_ioa(box1, box2, iou=False, eps=1e-7):
    """box1 (n, 4), box2 (m, 4) xyxy -> (n, m) intersection over the area of box2"""
    assert not iou
    ax1, ay1, ax2, ay2 = box1.T
    bx1, by1, bx2, by2 = box2.T
    iw = (np.minimum(ax2[:, None], bx2) - np.maximum(ax1[:, None], bx1)).clip(0)
    ih = (np.minimum(ay2[:, None], by2) - np.maximum(ay1[:, None], by1)).clip(0)
    return iw * ih / ((bx2 - bx1) * (by2 - by1) + eps)


# ---- drawContours(FILLED) -------------------------------------------------------------------------------------------------------------------------------------------------
def clip_line(width, height, p1, p2):
    """cv::clipLine on integers -> (visible, (x1, y1), (x2, y2))"""
    x1, y1, x2, y2 = int(p1[0]), int(p1[1]), int(p2[0]), int(p2[1])
    right, bottom = width - 1, height - 1
    c1 = (x1 < 0) + (x1 > right) * 2 + (y1 < 0) * 4 + (y1 > bottom) * 8
    c2 = (x2 < 0) + (x2 > right) * 2 + (y2 < 0) * 4 + (y2 > bottom) * 8
    if (c1 & c2) == 0 and (c1 | c2) != 0:
        if c1 & 12:
            a = 0 if c1 < 8 else bottom
            x1 += int(float(a - y1) * (x2 - x1) / (y2 - y1))
            y1 = a
            c1 = (x1 < 0) + (x1 > right) * 2
        if c2 & 12:
            a = 0 if c2 < 8 else bottom
            x2 += int(float(a - y2) * (x2 - x1) / (y2 - y1))
            y2 = a
            c2 = (x2 < 0) + (x2 > right) * 2
        if (c1 & c2) == 0 and (c1 | c2) != 0:
            if c1:
                a = 0 if c1 == 1 else right
                y1 += int(float(a - x1) * (y2 - y1) / (x2 - x1))
                x1 = a
                c1 = 0
            if c2:
                a = 0 if c2 == 1 else right
                y2 += int(float(a - x2) * (y2 - y1) / (x2 - x1))
                x2 = a
                c2 = 0
    return (c1 | c2) == 0, (x1, y1), (x2, y2)


def line_pixels(width, height, p1, p2) -> list:
    """the pixels of the 8-connected line p1 -- p2 on a width x height image: [(x, y), ...]"""
    ok, (x1, y1), (x2, y2) = clip_line(width, height, p1, p2)
    if not ok:
        return []
    if x2 < x1:   # left to right
        x1, y1, x2, y2 = x2, y2, x1, y1
    dx, dy = x2 - x1, abs(y2 - y1)
    sy = -1 if y2 < y1 else 1
    steep = dy > dx
    major, minor = (dy, dx) if steep else (dx, dy)
    err, out, x, y = major - 2 * minor, [], x1, y1
    for _ in range(major + 1):
        out.append((x, y))
        neg = err < 0
        err += -2 * minor + (2 * major if neg else 0)
        if steep:
            y, x = y + sy, x + (1 if neg else 0)
        else:
            x, y = x + 1, y + (sy if neg else 0)
    return out


def fill_mask(width, height, pts) -> np.ndarray:
    """drawContours([pts], -1, 1, FILLED) into a zero image -> (height, width) bool; pts (k, 2) integers, k >= 1"""
    pts = np.asarray(pts).astype(np.int64).reshape(-1, 2)
    mask = np.zeros((height, width), dtype=bool)
    edges, p0 = [], pts[-1]
    for p1 in pts:
        for x, y in line_pixels(width, height, p0, p1):
            mask[y, x] = True
        if p0[1] != p1[1]:
            (xa, ya), (xb, yb) = ((p0, p1) if p0[1] < p1[1] else (p1, p0))
            num, den = (int(xb) - int(xa)) << 16, int(yb) - int(ya)
            edges.append((int(ya), int(yb), int(xa) << 16, (abs(num) // den) * (1 if num >= 0 else -1)))   # the quotient truncates towards zero
        p0 = p1
    if edges:
        y0, y1, x0, dx = (np.array(v, dtype=np.int64) for v in zip(*edges))
        for y in range(max(int(y0.min()), 0), min(int(y1.max()), height)):
            act = (y0 <= y) & (y < y1)
            xs = np.sort(x0[act] + (y - y0[act]) * dx[act])
            for lo, hi in zip(xs[0::2].tolist(), xs[1::2].tolist()):
                a, b = (lo + 65535) >> 16, hi >> 16
                if a < width and b >= 0:
                    mask[y, max(a, 0) : min(b, width - 1) + 1] = True
    return mask


def draw_contours(im, contours, idx, color, thickness):
    """what the generator binds cv2.drawContours to"""
    assert idx == -1 and thickness == -1 and im.dtype == np.uint8
    for c in contours:
        assert c.dtype == np.int32
        im[fill_mask(im.shape[1], im.shape[0], c.reshape(-1, 2))] = color
    return im


def flip(im, code):
    """what the generator binds cv2.flip to"""
    assert code == 1
    return np.ascontiguousarray(im[:, ::-1])


# ---- copy_paste inside load_mosaic ------------------------------------------------------------------------------------------------------------------------------------------
def mosaic_rows(mo, labels, segments, hw):
    """labels4 and segments4 of a drawn mosaic as load_mosaic hands them to copy_paste -> (t (n, 5) float32 clipped, polys per row (None without a polygon))"""
    rows, polys = [], []
    for j, (padw, padh) in zip(mo.indices, mo.pad):
        lb = labels[j].copy()
        if lb.size:
            lb[:, 1:] = apc.xywhn2xyxy(lb[:, 1:], hw[j][1], hw[j][0], padw, padh)
            polys += [apc.canvas_polygon(p, hw[j][1], hw[j][0], padw, padh, mo.canvas) for p in segments[j]] if len(segments[j]) else [None] * len(lb)
        rows.append(lb)
    t = np.concatenate(rows, 0)
    np.clip(t[:, 1:], 0, mo.canvas, out=t[:, 1:])
    return t, polys


def copy_paste(t, polys, js, w):
    """The loop of copy_paste over the drawn js: label row j is paired with polygon j of the list of polygons (not the same object in a mosaic that mixes polygon
    images with box-only ones) -> dict(t: the grown labels, polys: per row (the appended rows' polygons last), accepted: [(slot, j, box (4,) float32)],
    ioa: per candidate the (rows,) float32 it was judged by, mask (w, w) bool: im_new)"""
    seglist = [p for p in polys if p is not None]
    assert all(0 <= j < len(seglist) for j in js)
    mask, accepted, ioas, added = np.zeros((w, w), dtype=bool), [], [], []
    for e, j in enumerate(js):
        label, segment = t[j], seglist[j]
        box = w - label[3], label[2], w - label[1], label[4]
        ioa = bbox_ioa(np.array([box], dtype=np.float32), t[:, 1:5])[0]
        assert ioa.dtype == np.float32
        ioas.append(ioa)
        if (ioa < 0.30).all():
            t = np.concatenate((t, [[label[0], *box]]), 0)
            added.append(np.concatenate((w - segment[:, 0:1], segment[:, 1:2]), 1))
            assert t.dtype == np.float32 and added[-1].dtype == np.float32
            mask |= fill_mask(w, w, segment.astype(np.int32))
            accepted.append((e, int(j), np.array(box, dtype=np.float32)))
    return dict(t=t, polys=list(polys) + added, accepted=accepted, ioa=ioas, mask=mask)


def paste_labels(item, labels, segments, hw, s):
    """The label path of one drawn item with copy-paste -> dict(targets (nl, 5) float32; per mosaic: words, accepted, masks (None where nothing was drawn for),
    rows (the grown labels before the filter), keep, ioa)"""
    out = dict(targets=None, words=[], accepted=[], masks=[], rows=[], keep=[], ioa=[])
    kept = []
    for mo in item.mosaics:
        if not item.mosaic:
            st = apc.polygon_labels(type(item)(item.index, [mo], None, None, False, False, False), labels, segments, hw, s)   # the letterbox branch: no paste
            t, keep, new, word, cp = st["rows"][0], st["keep"][0], st["new"][0], 0, dict(accepted=[], mask=None, ioa=[])
        else:
            t, polys = mosaic_rows(mo, labels, segments, hw)
            js = list(getattr(mo, "paste", ()) or ())
            cp = copy_paste(t, polys, js, mo.canvas) if js else dict(t=t, polys=polys, accepted=[], ioa=[], mask=None)
            t, polys, n = cp["t"], cp["polys"], len(cp["t"])
            word = (apc.PATH_NONZERO if any(p is not None and p.any() for p in polys) else 0) | (apc.PATH_LACKS if any(p is None for p in polys) else 0)
            new, keep = np.zeros((n, 4)), np.zeros(n, dtype=bool)
            if n:
                poly = word == apc.PATH_NONZERO
                new = np.array([apc.polygon_box(p, mo.M, s)[0] for p in polys]).reshape(n, 4) if poly else apc.corner_boxes(t[:, 1:5], mo.M, s)
                keep, _ = apc.candidates(t[:, 1:5], new, mo.scale, 0.01 if poly else 0.10)
        for key, v in (("words", word), ("accepted", cp["accepted"]), ("masks", cp["mask"]), ("rows", t.copy()), ("keep", keep), ("ioa", cp["ioa"])):
            out[key].append(v)
        t = t[keep]
        t[:, 1:5] = new[keep]
        kept.append(t)
    t = np.concatenate(kept, 0)
    if len(t):
        t[:, 1:5] = apc.xyxy2xywhn_clip(t[:, 1:5], s)
        if item.flipud:
            t[:, 2] = 1 - t[:, 2]
        if item.fliplr:
            t[:, 1] = 1 - t[:, 1]
    assert t.dtype == np.float32
    out["targets"] = t
    return out


def canvas_of(mo, images, mask=None):
    """the canvas of a drawn Mosaic (or the letterboxed image) and, with a mask, copy_paste's pixels: pixel (x, y) becomes pixel (w - 1 - x, y) of the canvas as it was
    before any paste wherever im_new[y, w - 1 - x] is set"""
    h = mo.canvas if getattr(mo, "canvas_h", None) is None else mo.canvas_h
    canvas = np.full((h, mo.canvas, 3), 114, dtype=np.uint8)
    for j, (x1a, y1a, x2a, y2a, x1b, y1b, x2b, y2b) in zip(mo.indices, mo.rects):
        canvas[y1a:y2a, x1a:x2a] = images[j][y1b:y2b, x1b:x2b]
    if mask is not None:
        result, i = canvas[:, ::-1].copy(), mask[:, ::-1]
        canvas[i] = result[i]
    return canvas


def item_image(item, images, masks, s) -> np.ndarray:
    """the image of one drawn item, (3, s, s) uint8 RGB: the canvases (with their pastes) through warp_affine_u8, mixup, the HSV tables, the flips, the transpose"""
    ims = [ac.warp_affine_u8(canvas_of(mo, images, mask), mo.M[:2], (s, s)) for mo, mask in zip(item.mosaics, masks)]
    im = ims[0]
    if len(ims) == 2:
        im = (im * item.ratio + ims[1] * (1 - item.ratio)).astype(np.uint8)
    if item.luts is not None:
        hsv = ac.bgr2hsv_u8(im)
        im = ac.hsv2bgr_u8(np.stack([item.luts[c][hsv[..., c]] for c in range(3)], -1))
    if item.flipud:
        im = np.flipud(im)
    if item.fliplr:
        im = np.fliplr(im)
    return np.ascontiguousarray(im.transpose((2, 0, 1))[::-1])


def batch_statement(items, images, labels, segments, hw, s):
    """a batch -> dict(im (count, 3, s, s) uint8, targets (nl, 6) float32, accepted: per (item, mosaic) slot [(slot, j, box)], masks: per (item, mosaic) slot,
    words (count, 2))"""
    ims, targets, accepted, masks, words = [], [], [], [], np.zeros((len(items), 2), dtype=np.int32)
    for b, it in enumerate(items):
        st = paste_labels(it, labels, segments, hw, s)
        targets.append(np.concatenate([np.full((len(st["targets"]), 1), b, dtype=np.float32), st["targets"]], 1))
        ims.append(item_image(it, images, st["masks"], s))
        for m in range(2):
            accepted.append(st["accepted"][m] if m < len(it.mosaics) else [])
            masks.append(st["masks"][m] if m < len(it.mosaics) else None)
            if m < len(it.mosaics):
                words[b, m] = st["words"][m]
    return dict(im=np.stack(ims), targets=np.concatenate(targets, 0).astype(np.float32).reshape(-1, 6), accepted=accepted, masks=masks, words=words)


def crc(a) -> int:
    return int(zlib.crc32(np.ascontiguousarray(a).tobytes()))


# ---- the situations the generator asserts (tests/golden/make_augment_copy_paste_golden.py) and the CPU test counts again ------------------------------------------------------
SITUATIONS = ("accepted_and_rejected", "rejected_by_appended_row", "k_zero", "mixed_mosaic_pairing", "polygon_path_paste", "touches_2s", "mixup_both_paste",
              "appended_survives", "appended_dropped")
def new_stats():
    return dict.fromkeys(SITUATIONS, 0)


def check_situations(stats):
    """every situation the copy-paste form can get wrong occurs under the seeds of the cases: an accepted and a rejected candidate in one mosaic; a candidate rejected
    only because of a row appended earlier; k == 0 with n > 0; an accepted paste in a mosaic that mixes polygon and box-only images, where label row j is not the row
    of polygon j (the box path); an accepted paste in an all-polygon mosaic on the polygon path; an accepted polygon that touches x = 2 S; a mixup item with accepted
    pastes in both mosaics; an appended row that survives box_candidates and one that does not"""
    missing = [k for k, v in stats.items() if not v]
    assert not missing, f"situations that do not occur: {missing} ({stats})"


def examine(item, st, labels, segments, hw, stats):
    """the threshold assertion and the situations of one item's statement `st` (cpc.paste_labels)"""
    if not item.mosaic:
        return
    both = 0
    for mo, word, acc, rows, keep, ioas in zip(item.mosaics, st["words"], st["accepted"], st["rows"], st["keep"], st["ioa"]):
        n = sum(len(segments[j]) for j in mo.indices)
        stats["k_zero"] += int(n > 0 and not mo.paste)
        t, polys = mosaic_rows(mo, labels, segments, hw)
        owner = [r for r, p in enumerate(polys) if p is not None]   # polygon j of the list belongs to label row owner[j]
        taken = {e for e, _, _ in acc}
        for v in ioas:
            assert (np.abs(v.astype(np.float64) - 0.30) > 1e-6).all(), "an ioa comparison lies within 1e-6 of 0.30"
        stats["accepted_and_rejected"] += int(0 < len(acc) < len(mo.paste))
        for e, v in enumerate(ioas):
            stats["rejected_by_appended_row"] += int(e not in taken and (v[: len(t)] < 0.30).all())
        for e, j, box in acc:
            stats["mixed_mosaic_pairing"] += int(bool(word & apc.PATH_LACKS) and owner[j] != j)
            stats["polygon_path_paste"] += int(word == apc.PATH_NONZERO)
            stats["touches_2s"] += int((polys[owner[j]][:, 0] == mo.canvas).any())
        appended = keep[len(t) :]
        stats["appended_survives"] += int(appended.any())
        stats["appended_dropped"] += int((~appended).any())
        both += int(len(acc) > 0)
    stats["mixup_both_paste"] += int(both == 2)


# ---- hand-made raster sets ------------------------------------------------------------------------------------------------------------------------------------------------
def raster_polygons() -> list:
    """normalised polygons that exercise the fill: concave, self-intersecting (a bow tie and a five-pointed star), 1203 vertices, horizontal edges (a rectangle and a
    staircase), vertices far outside the image (clipped onto 0 and 2 S), one and two vertices, and rings of 1024 and 1025 vertices: the raster keeps the first 1024
    edges of a polygon in LDS and forms the rest from the vertices, so these two and the 1203 lie on and on either side of that switch"""
    rs = np.random.RandomState(zlib.crc32(b"augment-copy-paste:raster"))
    ang = np.arange(5) * (4 * np.pi / 5)
    many = np.sort(rs.uniform(0, 2 * np.pi, 1203))
    return [np.asarray(p, dtype=np.float32) for p in (
        [[0.1, 0.1], [0.9, 0.15], [0.5, 0.4], [0.85, 0.9], [0.15, 0.8], [0.4, 0.45]],                        # concave
        [[0.1, 0.1], [0.9, 0.9], [0.9, 0.1], [0.1, 0.9]],                                                    # a bow tie
        np.stack([0.5 + 0.45 * np.sin(ang), 0.5 - 0.45 * np.cos(ang)], 1),                                   # a star: even-odd leaves its centre empty
        np.stack([0.5 + 0.4 * rs.uniform(0.6, 1.0, 1203) * np.cos(many), 0.5 + 0.4 * rs.uniform(0.6, 1.0, 1203) * np.sin(many)], 1),
        [[0.2, 0.25], [0.8, 0.25], [0.8, 0.75], [0.2, 0.75]],                                                # horizontal edges
        [[0.1, 0.9], [0.1, 0.6], [0.4, 0.6], [0.4, 0.3], [0.7, 0.3], [0.7, 0.1], [0.9, 0.1], [0.9, 0.9]],    # a staircase
        [[-10.0, -10.0], [10.0, -10.0], [10.0, 10.0], [0.5, 0.5]],                                            # clipped onto 0 and 2 S
        [[10.0, 0.3], [-10.0, 10.0], [0.3, -10.0]],
        [[0.35, 0.65]],
        [[0.2, 0.3], [0.9, 0.55]],
        *(np.stack([0.5 + 0.45 * rs.uniform(0.5, 1.0, k) * np.cos(np.arange(k) * (2 * np.pi / k)), 0.5 + 0.45 * rs.uniform(0.5, 1.0, k) * np.sin(np.arange(k) * (2 * np.pi / k))], 1)
          for k in (1024, 1025)),
    )]


def raster_set(s: int):
    """Four s x s images, every label row a tiny box (so that every mirrored box is accepted: the boxes are not derived from the polygons, which the reference's parser
    cannot produce -- the expectations are the statement's alone) with one of raster_polygons: 3 + 3 + 3 + 3 rows, so a mosaic of the four holds twelve polygons, more
    than a block has waves -> (images, labels, segments, hw)"""
    rs = np.random.RandomState(zlib.crc32(f"augment-copy-paste:set{s}".encode()))
    images = [rs.randint(0, 256, (s, s, 3)).astype(np.uint8) for _ in range(4)]
    polys, labels, segments, r = raster_polygons(), [], [], 0
    for n in (3, 3, 3, 3):
        lb = np.zeros((n, 5), dtype=np.float32)
        for q in range(n):
            lb[q] = (r % 3, 0.06 + 0.075 * r, 0.05 + 0.3 * q, 0.02, 0.02)
            r += 1
        labels.append(lb)
        segments.append(polys[r - n : r])
    return images, labels, segments, [(s, s)] * 4
