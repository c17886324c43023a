"""A/B of the COCO bbox evaluation behind `run_batches(save_json=True, anno_json=...)` (reference val.py:464-477) on synthetic inputs at val2017's scale (5 000 images,
80 categories, about 36 k annotations, about 1.5 M detections: 300 per image at conf_thres 0.001):
  (a) the host loops of pycocotools' COCOeval as tests/coco_eval_cases.py restates them (pure Python: far too slow for the whole set, so (a) runs on the first
      `--host-images` images and the device runs on the same subset beside it),
  (b) yolov3_amd.coco_eval.CocoEval.evaluate on the device, whole set and subset, with its host share split off: the jdict parse, the upload, the two launches, the read-back,
  (c) pycocotools itself on the subset and on the whole set, when it is importable,
interleaved rounds after a warm-up.  Run on the GPU machine under one time limit:

    timeout -k 10 900 python tools/coco_eval_ab.py --out profiles/coco_eval_ab.txt
"""
from __future__ import annotations

import argparse
import platform
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))


def cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return platform.processor() or "unknown"


def synth(n_img, n_cat, gt_per_img, det_per_img, seed=0):
    """-> (annotation dict, detections (N, 7) [image_id, category_id, x, y, w, h, score] rounded as save_one_json rounds).  A third of an image's detections are its
    ground truths, nudged; the rest are clutter; 2 % of the ground truths are crowds."""
    rng = np.random.default_rng(seed)
    img_ids = np.arange(1, n_img + 1) * 7 + 100
    n_gt = rng.poisson(gt_per_img, n_img).clip(0, 90)
    g_img = np.repeat(np.arange(n_img), n_gt)
    G = int(g_img.size)
    g_cat = rng.integers(0, n_cat, G) * (rng.random(G) < 0.5) + rng.integers(0, 5, G) * 1   # a few frequent categories, as in COCO
    g_cat = g_cat.clip(0, n_cat - 1)
    wh = np.exp(rng.normal(4.0, 1.0, (G, 2))).clip(4, 500)
    xy = rng.random((G, 2)) * (640 - wh).clip(1, None)
    g_box = np.round(np.concatenate((xy, wh), 1), 2)
    crowd = (rng.random(G) < 0.02).astype(int)
    area = np.round(g_box[:, 2] * g_box[:, 3] * rng.uniform(0.5, 1.0, G), 2)
    anno = dict(images=[dict(id=int(i)) for i in img_ids], categories=[dict(id=int(c + 1)) for c in range(n_cat)],
                annotations=[dict(id=i + 1, image_id=int(img_ids[g_img[i]]), category_id=int(g_cat[i] + 1), bbox=g_box[i].tolist(), area=float(area[i]), iscrowd=int(crowd[i]))
                             for i in range(G)])
    starts = np.concatenate(([0], np.cumsum(n_gt)))
    parts = []
    for i in range(n_img):
        k = det_per_img
        t = np.empty((k, 7))
        t[:, 0] = img_ids[i]
        n_near = min(k // 3, 4 * int(n_gt[i])) if n_gt[i] else 0
        if n_near:
            src = starts[i] + rng.integers(0, n_gt[i], n_near)
            t[:n_near, 1] = g_cat[src] + 1
            t[:n_near, 2:6] = g_box[src] + rng.normal(0, 4, (n_near, 4))
        t[n_near:, 1] = rng.integers(1, n_cat + 1, k - n_near)
        t[n_near:, 2:4] = rng.random((k - n_near, 2)) * 560
        t[n_near:, 4:6] = np.exp(rng.normal(3.5, 0.8, (k - n_near, 2)))
        t[:, 4:6] = t[:, 4:6].clip(1, None)
        t[:, 6] = np.where(np.arange(k) < n_near, rng.beta(2, 2, k), rng.beta(1, 12, k)).clip(0.001, 1)
        parts.append(t)
    dets = np.concatenate(parts)
    dets[:, 2:6] = np.round(dets[:, 2:6], 3)
    dets[:, 6] = np.round(dets[:, 6], 5)
    return anno, dets


def as_jdict(dets):
    return [{"image_id": int(r[0]), "category_id": int(r[1]), "bbox": r[2:6], "score": r[6]} for r in dets.tolist()]


def pycocotools_eval(anno, jdict, img_ids):
    import contextlib
    import copy
    import io

    from pycocotools.coco import COCO
    from pycocotools.cocoeval import COCOeval

    with contextlib.redirect_stdout(io.StringIO()):
        gt = COCO()
        gt.dataset = copy.deepcopy(anno)
        gt.createIndex()
        ev = COCOeval(gt, gt.loadRes(copy.deepcopy(jdict)), "bbox")
        ev.params.imgIds = list(img_ids)
        ev.evaluate()
        ev.accumulate()
        ev.summarize()
    return ev


def main():
    import coco_eval_cases as cc
    from yolov3_amd import CocoEval, CocoGroundTruth, coco_eval, ops

    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--images", type=int, default=5000)
    ap.add_argument("--categories", type=int, default=80)
    ap.add_argument("--dets-per-image", type=int, default=300)
    ap.add_argument("--host-images", type=int, default=100)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    try:
        import pycocotools  # noqa: F401
        have_pct = True
    except ImportError:
        have_pct = False

    dev = torch.device("cuda:0")
    anno, dets = synth(a.images, a.categories, 7.3, a.dets_per_image)
    jdict = as_jdict(dets)
    sub_ids = [im["id"] for im in anno["images"][: a.host_images]]
    sub_set = set(sub_ids)
    sub_anno = dict(images=anno["images"][: a.host_images], categories=anno["categories"], annotations=[x for x in anno["annotations"] if x["image_id"] in sub_set])
    sub_jdict = [d for d in jdict if d["image_id"] in sub_set]
    t0 = time.perf_counter()
    gt = CocoGroundTruth(anno, dev)
    ev = CocoEval(gt)
    torch.cuda.synchronize()
    setup = time.perf_counter() - t0
    ev_sub = CocoEval(gt, sub_ids)

    def clock(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t, r

    def device_split(e, jd):
        """evaluate() step by step, each step drained"""
        t_parse, cols = clock(lambda: e._columns(jd))
        t_up, up = clock(lambda: [coco_eval._upload(c, dev) for c in cols])
        t_match, rows = clock(lambda: ops.coco_match(*up, e._img_ids, gt.cat_ids_device, e._gt_box, e._gt_area, e._gt_crowd, e._gt_cat, e._gt_offsets, e._iou_thrs, e._area_rng,
                                                     e.max_dets[-1]))
        t_acc, out = clock(lambda: ops.coco_accumulate(rows, int(e.iou_thrs.size), e._rec_thrs, e._max_dets))
        t_read, _ = clock(lambda: torch.cat([o.view(-1) for o in out]).cpu().numpy())
        return dict(parse=t_parse, upload=t_up, match=t_match, accumulate=t_acc, read=t_read)

    times = {k: [] for k in ("host_sub", "dev_sub", "dev_all_jdict", "dev_all_array", "pct_sub", "pct_all")}
    splits = []
    equal = pct_equal = None
    for r in range(a.rounds + 1):   # round 0: warm-up
        th, want = clock(lambda: cc.evaluate(sub_anno, sub_jdict, sub_ids))
        td, res = clock(lambda: ev_sub.evaluate(sub_jdict))
        tj, full = clock(lambda: ev.evaluate(jdict))
        ta, full_a = clock(lambda: ev.evaluate(dets))
        split = device_split(ev, jdict)
        if have_pct:
            tps, p_sub = clock(lambda: pycocotools_eval(anno, sub_jdict, sub_ids))
            tpa, p_all = clock(lambda: pycocotools_eval(anno, jdict, gt.img_ids.tolist()))
        if r:
            times["host_sub"].append(th); times["dev_sub"].append(td); times["dev_all_jdict"].append(tj); times["dev_all_array"].append(ta)
            splits.append(split)
            if have_pct:
                times["pct_sub"].append(tps); times["pct_all"].append(tpa)
        equal = all(np.array_equal(getattr(res, k), want[k]) for k in ("precision", "recall", "scores")) and np.array_equal(res.stats, want["stats"]) \
            and np.array_equal(full.precision, full_a.precision) and np.array_equal(full.stats, full_a.stats)
        if have_pct:
            pct_equal = all(np.array_equal(getattr(full, k), p_all.eval[k]) for k in ("precision", "recall", "scores")) and np.array_equal(full.stats, p_all.stats) \
                and np.array_equal(res.precision, p_sub.eval["precision"])

    def row(label, ts):
        return f"{label:<66}" + "  ".join(f"{t * 1e3:10.2f}" for t in ts) + f"   median {statistics.median(ts) * 1e3:.2f} ms"

    med = {k: statistics.median(v) for k, v in times.items() if v}
    ms = {k: statistics.median(s[k] for s in splits) * 1e3 for k in splits[0]}
    total = sum(ms.values())
    lines = [f"coco_eval_ab: {a.images} images, {a.categories} categories, {len(anno['annotations'])} annotations, {len(jdict)} detections; subset for the host loops: "
             f"{a.host_images} images, {len(sub_anno['annotations'])} annotations, {len(sub_jdict)} detections; {a.rounds} interleaved rounds after one warm-up",
             f"device: {torch.cuda.get_device_name(0)}   host CPU: {cpu_model()}   pycocotools importable: {have_pct}",
             f"one-off: CocoGroundTruth + CocoEval (parse the annotation dict, group, upload): {setup * 1e3:.1f} ms",
             row("(a) host loops (tests/coco_eval_cases.py), subset:", times["host_sub"]),
             row("(b) CocoEval.evaluate(jdict), subset:", times["dev_sub"]),
             row("(b) CocoEval.evaluate(jdict), whole set:", times["dev_all_jdict"]),
             row("(b) CocoEval.evaluate((N, 7) array), whole set:", times["dev_all_array"])]
    if have_pct:
        lines += [row("(c) pycocotools loadRes + evaluate + accumulate + summarize, subset:", times["pct_sub"]),
                  row("(c) pycocotools, whole set:", times["pct_all"])]
    lines += [f"ratio on the subset (a) / (b): x{med['host_sub'] / med['dev_sub']:.1f}" + (f"   (c) / (b): subset x{med['pct_sub'] / med['dev_sub']:.1f}, whole set x{med['pct_all'] / med['dev_all_jdict']:.1f}"
                                                                                         if have_pct else ""),
              "split of one evaluate(jdict) on the whole set, each step drained (medians, ms): " + "  ".join(f"{k} {v:.2f}" for k, v in ms.items()),
              f"host share (jdict parse + upload): {100 * (ms['parse'] + ms['upload']) / total:.1f} %   device (match + accumulate): {ms['match'] + ms['accumulate']:.2f} ms   "
              f"with the (N, 7) array instead of the jdict the parse is a column split: whole call {med['dev_all_array'] * 1e3:.2f} ms",
              f"device arrays equal the host loops' on the subset, jdict and array forms equal: {equal}" + (f"   equal to pycocotools' (whole set and subset): {pct_equal}" if have_pct else ""),
              "whole-set stats: " + " ".join(f"{v:.4f}" for v in full.stats)]
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text)


if __name__ == "__main__":
    main()
