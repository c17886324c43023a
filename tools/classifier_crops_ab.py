"""What the device-side apply_classifier costs on one MI355X (csrc/crops.hip through yolov3_amd/crops.py), in interleaved rounds: a batch of --batch images of
--height x --width with about --detections detections in all, letterboxed to --imgsz.  The outputs are first checked equal to the NumPy statement of
tests/classifier_crops_cases.py (boxes, every crop, the kept rows); then every round times each arm once:

  classifier_boxes   y3_classifier_boxes
  scale_boxes        y3_scale_boxes on the box table
  crop_resize        y3_crop_resize in float32 and in float16, with the output GB/s beside a plain copy_ of the same bytes -- the floor of a kernel that writes them
  keep_matching      y3_keep_matching
  whole call         apply_classifier_batched end to end with a classifier that costs nothing (it hands back logits computed beforehand): uploads of the small tables,
                     the four launches, the one copy back, the host's own time -- wall clock around a synchronize

Medians over the rounds are printed and written.  There is no host arm: cv2 is not here, so nothing is compared with a cv2 build or timed against the reference's
host loop.  Run on the GPU machine under one time limit:

    timeout -k 10 300 python tools/classifier_crops_ab.py [--batch 32] [--detections 300] [--rounds 9] [--out profiles/classifier_crops_ab.txt]
"""
import argparse
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))


def build(args):
    """seeded images and detections in the letterboxed space: boxes of 20 .. 200 native pixels anywhere in the image, the edges included"""
    from oracle.yolo_oracle import synth_image_u8

    rng = np.random.RandomState(11)
    base = synth_image_u8(args.height, args.width, seed=77)
    ims = [np.ascontiguousarray(np.roll(base, (7 * i, 13 * i), (0, 1))) for i in range(args.batch)]
    gain = min(args.imgsz / args.height, args.imgsz / args.width)
    px, py = (args.imgsz - args.width * gain) / 2, (args.imgsz - args.height * gain) / 2
    counts = rng.multinomial(args.detections - args.batch, np.ones(args.batch) / args.batch) + 1
    x = []
    for n in counts:
        cx, cy = rng.uniform(0, args.width, n), rng.uniform(0, args.height, n)
        w, h = rng.uniform(20, 200, n), rng.uniform(20, 200, n)
        rows = np.stack([(cx - w / 2) * gain + px, (cy - h / 2) * gain + py, (cx + w / 2) * gain + px, (cy + h / 2) * gain + py, rng.uniform(0.3, 0.9, n), np.zeros(n)], 1)
        x.append(torch.from_numpy(rows.astype(np.float32)))
    return ims, x, [int(c) for c in counts]


def gpu_ms(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def wall_ms(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--detections", type=int, default=300)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--imgsz", type=int, default=640)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "classifier_crops_ab.txt"))
    args = ap.parse_args()

    import classifier_crops_cases as cc
    from yolov3_amd import DeviceImages, apply_classifier_batched, classifier_crops, ops
    from yolov3_amd.general import _gain_pad

    dev = torch.device("cuda")
    ims, x, counts = build(args)
    img1 = (args.imgsz, args.imgsz)
    bs, n = args.batch, sum(counts)
    rows = torch.zeros(bs, max(counts), 6)
    for i, d in enumerate(x):
        rows[i, : counts[i]] = d
    rows, counts_t = rows.to(dev), torch.tensor(counts, dtype=torch.int32, device=dev)
    images = DeviceImages(ims, dev)

    # ---- the check: boxes, every crop, the kept rows against the statement
    crops, boxes, prefix, status = classifier_crops(rows, counts_t, counts, img1, images, size=args.size)
    model = cc.ToyClassifier()
    want_boxes = [cc.scaled_boxes(d, im.shape, img1) for d, im in zip(x, ims)]
    want_u8 = [cc.crops_u8(im, b, args.size) for im, b in zip(ims, want_boxes)]
    want = torch.cat([cc.to_float(u) for u in want_u8], 0)
    assert status.tolist() == [0] and all(torch.equal(boxes[i, :c].cpu(), want_boxes[i]) for i, c in enumerate(counts)) and torch.equal(crops.cpu(), want)
    logits = model(want)
    pred = logits.argmax(1)
    cls = pred.clone()
    cls[1::3] = (cls[1::3] + 1) % cc.NC
    for i, c in enumerate(cls.float().split(counts)):   # every third row gets a class the classifier does not confirm
        rows[i, : counts[i], 5] = c.to(dev)
    logits_dev = logits.to(dev)
    kept, kept_t, kept_n = apply_classifier_batched(rows, counts_t, counts, lambda c: logits_dev, img1, images, size=args.size, dtype=torch.float32)
    off = 0
    for i, c in enumerate(counts):
        d = rows[i, :c].cpu()
        assert torch.equal(kept[i, : kept_n[i]].cpu(), d[d[:, 5].long() == pred[off : off + c]])
        off += c
    checked = f"checked equal to the statement: {n} boxes, {n} crops of {args.size} x {args.size}, {sum(kept_n)} kept rows of {n}"

    # ---- the arms
    params = torch.tensor([[*_gain_pad(img1, im.shape, None), float(im.shape[1]), float(im.shape[0])] for im in ims], dtype=torch.float32, device=dev)
    pred_dev = pred.to(dev)
    scratch = boxes.clone()
    out32 = torch.empty(n, 3, args.size, args.size, dtype=torch.float32, device=dev)
    out16 = torch.empty(n, 3, args.size, args.size, dtype=torch.float16, device=dev)
    src32, src16 = torch.rand_like(out32), torch.rand_like(out16)
    word = torch.zeros(1, dtype=torch.int32, device=dev)
    arms = {
        "classifier_boxes": (gpu_ms, lambda: ops.classifier_boxes(rows, counts_t)),
        "scale_boxes": (gpu_ms, lambda: ops.scale_boxes_raw(scratch, scratch.stride(0), 4, counts_t, bs, scratch.shape[1], params)),
        "crop_resize fp32": (gpu_ms, lambda: ops.crop_resize(images.arena, images.records, boxes, counts_t, prefix, n, args.size, torch.float32, word, out32)),
        "copy_ fp32": (gpu_ms, lambda: out32.copy_(src32)),
        "crop_resize fp16": (gpu_ms, lambda: ops.crop_resize(images.arena, images.records, boxes, counts_t, prefix, n, args.size, torch.float16, word, out16)),
        "copy_ fp16": (gpu_ms, lambda: out16.copy_(src16)),
        "keep_matching": (gpu_ms, lambda: ops.keep_matching(rows, counts_t, prefix, pred_dev, boxes, images.arena, images.records)),
        "whole call": (wall_ms, lambda: apply_classifier_batched(rows, counts_t, counts, lambda c: logits_dev, img1, images, size=args.size, dtype=torch.float32)),
    }
    for timer, fn in arms.values():   # warm-up
        timer(fn, 3)
    times = {k: [] for k in arms}
    for _ in range(args.rounds):
        for k, (timer, fn) in arms.items():
            times[k].append(timer(fn, args.iters))
    assert word.tolist() == [0]

    lines = [f"classifier_crops_ab: {torch.cuda.get_device_name(0)}, batch {bs} of {args.height} x {args.width}, {n} detections, crops {args.size} x {args.size}, "
             f"{args.rounds} interleaved rounds of {args.iters} calls, medians (min .. max)", checked, ""]
    for k, v in times.items():
        med = statistics.median(v)
        line = f"  {k:18s} {med * 1e3:9.1f} us   ({min(v) * 1e3:.1f} .. {max(v) * 1e3:.1f})"
        if "fp32" in k or "fp16" in k:
            line += f"   {(out32 if 'fp32' in k else out16).numel() * (4 if 'fp32' in k else 2) / med / 1e6:7.1f} GB/s written"
        lines.append(line)
    lines += ["", "No arm for the reference's host loop: cv2 is not installed here, nothing was compared with a cv2 build.",
              "y3_letterbox_u8 is not timed: with the coefficient function in csrc/y3_resize_u8.h, letterbox_u8_kernel compiles to the instruction list it had before "
              "(198 instructions, compared line by line in the hipcc -S output for gfx950)."]
    text = "\n".join(lines) + "\n"
    print(text)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(text)


if __name__ == "__main__":
    main()
