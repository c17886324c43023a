"""Shared inputs and the NumPy statement of the classifier-crop tests (tests/test_classifier_crops_cpu.py, tests/test_gpu_classifier_crops.py,
tests/golden/make_classifier_crops_golden.py): reference utils/general.py:827-859 apply_classifier, step by step.  Not a test file.

The statement is pinned by the unmodified reference where the fixture is generated (every cutout, every classifier input, every kept row); the one piece the reference
cannot supply here, cv2.resize, is oracle.yolo_oracle.resize_linear_u8 -- the restatement that already backs y3_letterbox_u8 and that no cv2 build has checked.

Five entries, letterboxed to 320 x 320: three images of 97 x 151, 200 x 120 and 300 x 260 (h x w; row bytes that are no multiples of 4, one image larger than 224 on both
axes so that a cutout shrinks) with 7, 8 and 9 detections, one image without detections and one None entry.  check_situations lists what the detections must reach.
"""
from __future__ import annotations

import hashlib

import numpy as np
import torch
from torch import nn

from oracle import upstream
from oracle.yolo_oracle import resize_linear_u8, scale_boxes, synth_image_u8

IMG1 = (320, 320)
SIZE = 224
NC = 4
SHAPES = [(97, 151), (200, 120), (300, 260), (33, 47), (20, 20)]   # (h, w); the last two: no detections, a None entry

# per image the detections as native (cx, cy, w, h); build_detections moves them into the letterboxed space and jitters them by a seeded fraction of a pixel
NATIVE = [
    [(75, 48, 30, 20), (8, 50, 12, 18), (70, 5, 20, 8), (146, 60, 10, 10), (40, 93, 14, 10), (75, 48, 100, 80), (155, 30, 4, 4)],
    [(60, 100, 40, 60), (10, 20, 15, 15), (110, 190, 20, 30), (60, 100, 110, 190), (30, 150, 25, 12), (90, 40, 9, 40), (60, 60, 50, 50), (45, 170, 33, 21)],
    [(10, 150, 20, 190), (130, 150, 250, 290), (130, 150, 100, 150), (200, 60, 40, 30), (250, 280, 30, 30), (50, 250, 60, 20), (128.3, 77.7, 12, 12), (90, 200, 45, 80),
     (180, 170, 70, 66)],
    [],
    None,
]
FULL_CROPS = [(0, 6), (2, 1)]   # (entry, detection) of the crops the fixture stores whole: the 6-pixel cutout, and the whole 300 x 260 image shrunk


class ToyClassifier(nn.Module):
    """A fixed, seedless classifier: the logits are a smooth function of the three plane means.  forward records its inputs."""

    def __init__(self):
        super().__init__()
        self.w = nn.Parameter(torch.tensor([[5.0, -3.0, 2.0, -4.0], [-2.0, 4.0, -5.0, 3.0], [3.0, 2.0, 4.0, -2.0]]), requires_grad=False)
        self.b = nn.Parameter(torch.tensor([0.3, 1.1, 2.0, 2.9]), requires_grad=False)
        self.seen = []

    def forward(self, x):
        self.seen.append(x)
        m = x.float().mean((2, 3))
        return torch.sin(m @ self.w.float() * 3.0 + self.b.float())


def images():
    return [synth_image_u8(h, w, seed=500 + i) for i, (h, w) in enumerate(SHAPES)]


def _gain_pad(shape0):
    gain = min(IMG1[0] / shape0[0], IMG1[1] / shape0[1])
    return gain, (IMG1[1] - shape0[1] * gain) / 2, (IMG1[0] - shape0[0] * gain) / 2


def build_detections():
    """per entry an (n, 6) fp32 tensor [x1, y1, x2, y2, conf, 0] in the letterboxed space, an empty one, or None; the class column is set by build_case"""
    rng = np.random.RandomState(20240611)
    out = []
    for shape0, boxes in zip(SHAPES, NATIVE):
        if boxes is None:
            out.append(None)
            continue
        gain, px, py = _gain_pad(shape0)
        rows = np.zeros((len(boxes), 6), dtype=np.float64)
        for j, (cx, cy, w, h) in enumerate(boxes):
            jit = rng.uniform(-0.5, 0.5, 4)
            rows[j, :4] = np.array([(cx - w / 2) * gain + px, (cy - h / 2) * gain + py, (cx + w / 2) * gain + px, (cy + h / 2) * gain + py]) + jit
            rows[j, 4] = 0.95 - 0.07 * j - 0.01 * rng.uniform()
        out.append(torch.from_numpy(rows.astype(np.float32)).reshape(-1, 6))
    return out


# ---- the statement ------------------------------------------------------------------------------------------------------------------------
def classifier_boxes(det, gain=1.3, pad=30, square=True):
    """d[:, :4] of reference utils/general.py:836-839 after `.long()`, as fp32: det (n, 6) fp32 -> (n, 4)"""
    b = upstream.xyxy2xywh(det[:, :4].clone())
    if square:
        b[:, 2:] = b[:, 2:].max(1)[0].unsqueeze(1)
    b[:, 2:] = b[:, 2:] * gain + pad
    return upstream.xywh2xyxy(b).long().float()


def scaled_boxes(det, shape0, img1=IMG1):
    """... and after scale_boxes(img.shape[2:], d[:, :4], im0[i].shape) (:842)"""
    return scale_boxes(img1, classifier_boxes(det), shape0)


def cutouts(im, boxes):
    """im0[i][int(y1):int(y2), int(x1):int(x2)] per row of the scaled boxes (:848)"""
    return [im[int(b[1]) : int(b[3]), int(b[0]) : int(b[2])] for b in boxes]


def crops_u8(im, boxes, size=SIZE):
    """cv2.resize(cutout, (size, size)) per row (:849) -> uint8 (n, size, size, 3), BGR as the source"""
    return np.stack([resize_linear_u8(c, size, size) for c in cutouts(im, boxes)], 0)


def to_float(u8):
    """im[:, :, ::-1].transpose(2, 0, 1), float32, /= 255 (:851-853) for a stack of crops -> (n, 3, size, size) fp32 tensor"""
    return torch.from_numpy(np.ascontiguousarray(u8[..., ::-1].transpose(0, 3, 1, 2))).float() / 255


def statement(ims, x, size=SIZE, classifier=None):
    """every step for every entry -> dict of per-entry lists: boxes (n, 4) fp32, crops uint8 (n, size, size, 3), logits (n, NC), pred (n,) int64, kept (m, 6); None
    for an entry without detections"""
    classifier = classifier or ToyClassifier()
    out = dict(boxes=[], crops=[], logits=[], pred=[], kept=[])
    for im, d in zip(ims, x):
        if d is None or not len(d):
            for v in out.values():
                v.append(None)
            continue
        boxes = scaled_boxes(d, im.shape)
        u8 = crops_u8(im, boxes, size)
        logits = classifier(to_float(u8))
        pred = logits.argmax(1)
        out["boxes"].append(boxes)
        out["crops"].append(u8)
        out["logits"].append(logits)
        out["pred"].append(pred)
        out["kept"].append(d[d[:, 5].long() == pred])
    return out


def build_case():
    """(images, x): the class column holds the toy classifier's class of the row's crop, except on every third row, which the filter must drop"""
    ims, x = images(), build_detections()
    st = statement(ims, x)
    for d, pred in zip(x, st["pred"]):
        if pred is not None:
            cls = pred.clone()
            cls[1::3] = (cls[1::3] + 1) % NC
            d[:, 5] = cls.float()
    return ims, x


def sha(a: np.ndarray) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def check_situations(ims, x, st):
    """the situations the case exists for; AssertionError names the one that is missing"""
    seen = dict(left=False, top=False, right=False, bottom=False, full_side=False, enlarge_and_shrink=False, under_8=False, fraction=False)
    for im, d, boxes, logits, kept in zip(ims, x, st["boxes"], st["logits"], st["kept"]):
        if boxes is None:
            continue
        h0, w0 = im.shape[:2]
        gain, px, py = _gain_pad(im.shape)
        raw = (classifier_boxes(d) - torch.tensor([px, py, px, py], dtype=torch.float32)) / gain   # the same boxes, not clipped
        for b, r in zip(boxes.tolist(), raw.tolist()):
            x1, y1, x2, y2 = (int(v) for v in b)
            w, h = x2 - x1, y2 - y1
            assert w >= 1 and h >= 1, "an empty cutout"
            seen["left"] |= r[0] < 0
            seen["top"] |= r[1] < 0
            seen["right"] |= r[2] > w0
            seen["bottom"] |= r[3] > h0
            seen["full_side"] |= w == w0 or h == h0
            seen["enlarge_and_shrink"] |= (w < SIZE < h) or (h < SIZE < w)
            seen["under_8"] |= w < 8 or h < 8
            seen["fraction"] |= any(v - int(v) > 0.5 for v in b)
        assert 0 < len(kept) < len(d), "an image needs a kept and a dropped row"
        top2 = logits.topk(2, 1).values
        assert float((top2[:, 0] - top2[:, 1]).min()) >= 1e-3, "two logits closer than 1e-3"
    missing = [k for k, v in seen.items() if not v]
    assert not missing, f"situations not reached: {missing}"
    assert any(s[0] > SIZE and s[1] > SIZE for s in SHAPES) and sum(d is None for d in x) == 1 and sum(d is not None and not len(d) for d in x) == 1


# ---- Detections.crop ----------------------------------------------------------------------------------------------------------------------
def save_one_box(xyxy, im, gain=1.02, pad=10, square=False, BGR=False):
    """The crop of upstream ultralytics.utils.plotting.save_one_box without its file half -> (crop, [x1, y1, x2, y2]).  RESTATED from the published definition and
    NOT PINNED (the ultralytics package is un-vendored): xyxy2xywh, optionally the square, `* gain + pad`, xywh2xyxy, .long(), clip_boxes to the image, then
    im[y1:y2, x1:x2, ::(1 if BGR else -1)].  fp32 throughout, as the tensor arithmetic of the original."""
    b = np.asarray(xyxy, dtype=np.float32).reshape(4)
    cx, cy, w, h = (b[0] + b[2]) / np.float32(2), (b[1] + b[3]) / np.float32(2), b[2] - b[0], b[3] - b[1]
    if square:
        w = h = max(w, h)
    w, h = w * np.float32(gain) + np.float32(pad), h * np.float32(gain) + np.float32(pad)
    box = [int(cx - w / np.float32(2)), int(cy - h / np.float32(2)), int(cx + w / np.float32(2)), int(cy + h / np.float32(2))]   # int(): truncation, as .long()
    box = [min(max(box[0], 0), im.shape[1]), min(max(box[1], 0), im.shape[0]), min(max(box[2], 0), im.shape[1]), min(max(box[3], 0), im.shape[0])]
    return im[box[1] : box[3], box[0] : box[2], :: (1 if BGR else -1)], box
