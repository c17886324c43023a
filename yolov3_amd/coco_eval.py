"""COCO bbox AP / AR of a run's COCO-JSON on the device: what reference val.py:464-477 asks of pycocotools (COCO(anno_json), loadRes(pred_json), COCOeval(..., "bbox"),
evaluate / accumulate / summarize) without pycocotools.

    gt = CocoGroundTruth("instances_val2017.json", "cuda")            # parsed and uploaded once
    res = CocoEval(gt).evaluate(jdict)                                 # or "predictions.json", or an (N, 7) array [image_id, category_id, x, y, w, h, score]
    map, map50 = res.stats[:2]                                         # val.py:477
    print("\\n".join(res.summarize()))

The matching of every (image, category) pair and the accumulation over every (threshold, category, area range, maxDets) cell run through csrc/coco_eval.hip
(y3_coco_match / y3_coco_accumulate) in fp64 and pycocotools' operation order: `precision`, `recall` and `scores` are its arrays bit for bit.  The host parses the
detections into columns, groups the ground truth by (image, category) once per CocoEval, and takes the twelve means of `summarize` with NumPy over the arrays the device
returns (one copy), exactly as pycocotools does.  The evaluator reads the ROUNDED values of the jdict (`round(x, 3)`, `round(conf, 5)`): what pycocotools reads from the file.

Differences from pycocotools, all deliberate:
  * boxes only (iouType "bbox", useCats = 1); image and category ids are integers;
  * a detection is matched when it has a ground truth (pycocotools records the ground truth's id, so an annotation with id 0 reads as "unmatched" there);
  * `max_dets` is sorted ascending (pycocotools reads maxDets[-1] as the cap and is wrong for an unsorted list);
  * there is no CPU path.
"""
from __future__ import annotations

import itertools
import json
from pathlib import Path

import numpy as np
import torch

from . import ops

_AREA_NAMES = ("all", "small", "medium", "large")
# (AP?, IoU or None, area, index into max_dets) of the twelve lines, in pycocotools' order
_SUMMARY = ((1, None, "all", -1), (1, .5, "all", -1), (1, .75, "all", -1), (1, None, "small", -1), (1, None, "medium", -1), (1, None, "large", -1),
            (0, None, "all", 0), (0, None, "all", 1), (0, None, "all", 2), (0, None, "small", -1), (0, None, "medium", -1), (0, None, "large", -1))


def _device(device, what: str) -> torch.device:
    if device is None and not torch.cuda.is_available():
        raise RuntimeError(f"{what}: no CPU / PyTorch fallback; the yolov3_amd hot path runs only on an MI355X (HIP) device.")
    device = torch.device(device if device is not None else "cuda")
    ops.require_gpu(torch.empty(0, device=device), what)
    return device


def _upload(a: np.ndarray, device) -> torch.Tensor:
    """every host -> device copy of this module"""
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _ids(values, what: str) -> np.ndarray:
    """integer ids as int64 (a float that is an integer is accepted: the (N, 7) form carries them as fp64)"""
    try:
        a = np.asarray(values)
        if a.dtype.kind not in "iuf":
            raise TypeError
        out = a.astype(np.int64)
        if a.dtype.kind == "f" and not np.array_equal(out.astype(a.dtype), a):
            raise TypeError
    except (TypeError, ValueError, OverflowError):
        raise ValueError(f"{what} must be integers") from None
    return out.reshape(-1)


class CocoGroundTruth:
    """A COCO annotation file (a path, or its dict with `images`, `annotations`, `categories`) as columns: .img_ids / .cat_ids sorted and unique (int64 NumPy), and per
    annotation, in file order, image id, category id, bbox [x, y, w, h], `area` and `iscrowd` (a missing `iscrowd` counts as 0; an `ignore` field is not read:
    pycocotools overwrites it with `iscrowd`).  The id lists are uploaded once; `CocoEval` uploads the grouped annotations once per image list."""

    def __init__(self, anno, device=None):
        self.device = _device(device, "CocoGroundTruth")
        if not isinstance(anno, dict):
            with open(anno) as f:
                anno = json.load(f)
        for key in ("images", "annotations", "categories"):
            if key not in anno:
                raise ValueError(f"CocoGroundTruth: the annotation file has no '{key}'")
        self.img_ids = np.unique(_ids([im["id"] for im in anno["images"]], "image ids"))
        self.cat_ids = np.unique(_ids([c["id"] for c in anno["categories"]], "category ids"))
        if self.img_ids.size == 0 or self.cat_ids.size == 0:
            raise ValueError("CocoGroundTruth: no images or no categories")
        anns = anno["annotations"]
        self.ann_img = _ids([a["image_id"] for a in anns], "image_id")
        self.ann_cat = _ids([a["category_id"] for a in anns], "category_id")
        self.ann_box = np.array([a["bbox"] for a in anns], dtype=np.float64).reshape(-1, 4)
        self.ann_area = np.array([a["area"] for a in anns], dtype=np.float64).reshape(-1)
        self.ann_crowd = np.array([1 if a.get("iscrowd", 0) else 0 for a in anns], dtype=np.uint8).reshape(-1)
        self.cat_ids_device = _upload(self.cat_ids, self.device)


def _positions(sorted_ids: np.ndarray, values: np.ndarray) -> np.ndarray:
    """position of every value in the sorted unique ids, -1 where it is not among them"""
    pos = np.searchsorted(sorted_ids, values)
    pos[pos == sorted_ids.size] = 0
    return np.where(sorted_ids[pos] == values, pos, -1) if sorted_ids.size else np.full(values.shape, -1)


class CocoResult:
    """.precision (T, R, K, A, M), .recall (T, K, A, M), .scores (T, R, K, A, M): pycocotools' COCOeval.eval arrays (NumPy fp64, -1 = no ground truth);
    .stats: the twelve numbers of COCOeval.summarize; .summarize(): its twelve lines."""

    def __init__(self, precision, recall, scores, iou_thrs, max_dets, area_names):
        self.precision, self.recall, self.scores = precision, recall, scores
        self.iou_thrs, self.max_dets, self.area_names = iou_thrs, max_dets, area_names
        self.stats, self._lines = self._summary()

    def _cell(self, ap, iou, area, mi):
        """_summarize of pycocotools: np.mean of the selected cells that are > -1, or -1"""
        a, m = self.area_names.index(area), range(len(self.max_dets))[mi]
        s = self.precision[:, :, :, a, m] if ap else self.recall[:, :, a, m]
        if iou is not None:
            s = s[np.where(iou == self.iou_thrs)[0]]
        mean = -1 if len(s[s > -1]) == 0 else np.mean(s[s > -1])
        iou_str = "{:0.2f}:{:0.2f}".format(self.iou_thrs[0], self.iou_thrs[-1]) if iou is None else "{:0.2f}".format(iou)
        line = " {:<18} {} @[ IoU={:<9} | area={:>6s} | maxDets={:>3d} ] = {:0.3f}".format("Average Precision" if ap else "Average Recall", "(AP)" if ap else "(AR)", iou_str, area,
                                                                                         self.max_dets[m], mean)
        return mean, line

    def _summary(self):
        if tuple(self.area_names) != _AREA_NAMES or len(self.max_dets) != 3:   # summarize is defined for the four named ranges and three maxDets
            return None, None
        cells = [self._cell(*row) for row in _SUMMARY]
        return np.array([c[0] for c in cells]), [c[1] for c in cells]

    def summarize(self):
        if self._lines is None:
            raise ValueError("summarize needs the default area ranges and three max_dets")
        return list(self._lines)


class CocoEval:
    """COCOeval(gt, ., "bbox") with pycocotools' Params: iou_thrs np.linspace(.5, .95, 10), rec_thrs np.linspace(0, 1, 101), max_dets (1, 10, 100), area_rng all / small /
    medium / large (bounds inclusive).  `img_ids`: the images to evaluate (made unique and sorted); None = every image of the file.  The ground truth of those images is
    grouped by (image, category) in file order and uploaded here, once."""

    def __init__(self, gt: CocoGroundTruth, img_ids=None, iou_thrs=None, rec_thrs=None, max_dets=(1, 10, 100), area_rng=None):
        if not isinstance(gt, CocoGroundTruth):
            raise TypeError("CocoEval expects a CocoGroundTruth")
        self.gt, dev = gt, gt.device
        self.iou_thrs = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True) if iou_thrs is None else np.asarray(iou_thrs, dtype=np.float64).reshape(-1)
        self.rec_thrs = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True) if rec_thrs is None else np.asarray(rec_thrs, dtype=np.float64).reshape(-1)
        self.max_dets = sorted(int(m) for m in max_dets)
        self.area_names = _AREA_NAMES if area_rng is None else tuple(str(i) for i in range(len(area_rng)))
        self.area_rng = np.array([[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]] if area_rng is None else area_rng, dtype=np.float64).reshape(-1, 2)
        if not (1 <= self.iou_thrs.size <= 16 and 1 <= self.area_rng.shape[0] <= 8 and 1 <= len(self.max_dets) <= 8 and 1 <= self.rec_thrs.size <= 1024):
            raise ValueError("CocoEval: 1 .. 16 IoU thresholds, 1 .. 8 area ranges, 1 .. 8 max_dets and 1 .. 1024 recall samples are supported")
        if self.max_dets[0] < 1 or not (np.isfinite(self.iou_thrs).all() and np.isfinite(self.rec_thrs).all()) or np.isnan(self.area_rng).any():
            raise ValueError("CocoEval: max_dets must be positive, the thresholds finite")
        self.img_ids = gt.img_ids if img_ids is None else np.unique(_ids(list(img_ids), "img_ids"))
        if self.img_ids.size == 0:
            raise ValueError("CocoEval: no images to evaluate")
        n_img, K = int(self.img_ids.size), int(gt.cat_ids.size)
        if n_img * K >= 2 ** 31 - 1:
            raise ValueError("CocoEval: images x categories must stay below 2^31 - 1")
        # the ground truth of the chosen images, grouped by (image position, category position), file order inside a pair
        ip, kp = _positions(self.img_ids, gt.ann_img), _positions(gt.cat_ids, gt.ann_cat)
        pair = np.where((ip >= 0) & (kp >= 0), ip * K + kp, -1)
        order = np.argsort(pair, kind="stable")
        order = order[pair[order] >= 0]
        offsets = np.zeros(n_img * K + 1, dtype=np.int64)
        np.cumsum(np.bincount(pair[order], minlength=n_img * K), out=offsets[1:])
        self.n_gt = int(order.size)
        self._img_ids = _upload(self.img_ids, dev)
        self._gt_box = _upload(gt.ann_box[order], dev)
        self._gt_area = _upload(gt.ann_area[order], dev)
        self._gt_crowd = _upload(gt.ann_crowd[order], dev)
        self._gt_cat = _upload(kp[order].astype(np.int32), dev)
        self._gt_offsets = _upload(offsets.astype(np.int32), dev)
        self._iou_thrs, self._rec_thrs = _upload(self.iou_thrs, dev), _upload(self.rec_thrs, dev)
        self._area_rng, self._max_dets = _upload(self.area_rng, dev), _upload(np.array(self.max_dets, dtype=np.int32), dev)

    def _columns(self, dets):
        """the three forms of `dets` -> (image ids int64, category ids int64, boxes fp64 (N, 4), scores fp64) on the host"""
        if isinstance(dets, (str, Path)):
            with open(dets) as f:
                dets = json.load(f)
        if isinstance(dets, np.ndarray):
            if dets.ndim != 2 or dets.shape[1] != 7:
                raise ValueError("CocoEval.evaluate: an array of detections is (N, 7) [image_id, category_id, x, y, w, h, score]")
            t = dets.astype(np.float64, copy=False)
            return _ids(t[:, 0], "image_id"), _ids(t[:, 1], "category_id"), t[:, 2:6], t[:, 6]
        dets = list(dets)
        img = _ids([d["image_id"] for d in dets], "image_id")
        cat = _ids([d["category_id"] for d in dets], "category_id")
        box = np.fromiter(itertools.chain.from_iterable(d["bbox"] for d in dets), dtype=np.float64)   # (np.array over 1.5 M four-element lists takes twice as long)
        if box.size != 4 * len(dets):
            raise ValueError("CocoEval.evaluate: every bbox is [x, y, w, h]")
        return img, cat, box.reshape(-1, 4), np.fromiter((d["score"] for d in dets), dtype=np.float64, count=len(dets))

    def evaluate(self, dets) -> CocoResult:
        """evaluate + accumulate + summarize for `dets`: the jdict list of save_one_json / save_json_batched, a path to such a JSON, or an (N, 7) array.  A detection whose
        image is not in the annotation file raises ValueError (pycocotools' loadRes asserts); one whose image is outside `img_ids`, or whose category is not in the
        file, takes no part."""
        img, cat, box, score = self._columns(dets)
        if img.size and not np.isin(img, self.gt.img_ids).all():
            raise ValueError("Results do not correspond to current coco set")   # loadRes' own message
        dev = self.gt.device
        rows = ops.coco_match(_upload(img, dev), _upload(cat, dev), _upload(box, dev), _upload(score, dev), self._img_ids, self.gt.cat_ids_device, self._gt_box, self._gt_area,
                              self._gt_crowd, self._gt_cat, self._gt_offsets, self._iou_thrs, self._area_rng, self.max_dets[-1])
        precision, recall, scores = ops.coco_accumulate(rows, int(self.iou_thrs.size), self._rec_thrs, self._max_dets)
        block = torch.cat((precision.view(-1), scores.view(-1), recall.view(-1))).cpu().numpy()   # the one read
        n = precision.numel()
        return CocoResult(block[:n].reshape(precision.shape), block[2 * n:].reshape(recall.shape), block[n : 2 * n].reshape(precision.shape), self.iou_thrs, self.max_dets,
                          self.area_names)
