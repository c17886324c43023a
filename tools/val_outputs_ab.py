"""A/B of what `--save-txt --save-conf --save-json` costs per batch after NMS (bs 32, val settings: conf 0.001, IoU 0.6, 300 rows per image;
oracle.yolo_oracle.synth_predictions, seed 5):
  (a) the per-image, per-box loop the way reference val.py writes it: `.tolist()` of every image's rows, one small tensor, one division and one open() per detection,
  (b) yolov3_amd.outputs.save_txt_batched + save_json_batched: one launch and one device->host copy per writer, then host formatting,
interleaved, five rounds each after a warm-up, into fresh directories (both append).  Run on the GPU machine under one time limit:

    timeout -k 10 600 python tools/val_outputs_ab.py --out profiles/val_outputs_ab.txt
"""
from __future__ import annotations

import argparse
import platform
import statistics
import sys
import tempfile
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return platform.processor() or "unknown"


def per_box_loop(dets, shapes, paths, folder, jdict, class_map):
    """val.py:379-413 for one batch: per image `predn.tolist()`, per box a (1, 4) tensor -> xywh / gn -> one line appended to the image's file; the JSON entries from
    one xywh tensor per image"""
    for predn, shape, path in zip(dets, shapes, paths):
        if predn.shape[0] == 0:
            continue
        gn = torch.tensor(shape)[[1, 0, 1, 0]]
        file = folder / f"{Path(path).stem}.txt"
        for *xyxy, conf, cls in predn.tolist():
            b = torch.tensor(xyxy).view(1, 4)
            xywh = (torch.cat(((b[:, :2] + b[:, 2:]) / 2, b[:, 2:] - b[:, :2]), 1) / gn).view(-1).tolist()
            line = (cls, *xywh, conf)
            with open(file, "a") as f:
                f.write(("%g " * len(line)).rstrip() % line + "\n")
        stem = Path(path).stem
        image_id = int(stem) if stem.isnumeric() else stem
        box = torch.cat(((predn[:, :2] + predn[:, 2:4]) / 2, predn[:, 2:4] - predn[:, :2]), 1)
        box[:, :2] -= box[:, 2:] / 2
        for p, b in zip(predn.tolist(), box.tolist()):
            jdict.append({"image_id": image_id, "category_id": class_map[int(p[5])], "bbox": [round(x, 3) for x in b], "score": round(p[4], 5)})


def main():
    from oracle import yolo_oracle as yo
    from yolov3_amd import coco80_to_coco91_class, non_max_suppression_batched, outputs

    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--bs", type=int, default=32)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    pred = yo.synth_predictions(bs=a.bs, n_rows=25200, nc=80, seed=5).to(dev)
    rows, counts_t, counts = non_max_suppression_batched(pred, 0.001, 0.6, None, False, True, 300)
    shapes = [(480, 640) if i % 2 else (427, 640) for i in range(a.bs)]
    paths = [f"{1000 + i:012d}.jpg" for i in range(a.bs)]
    class_map = coco80_to_coco91_class()
    dets = [rows[i, :c] for i, c in enumerate(counts)]
    torch.cuda.synchronize()

    def run(which, folder):
        jdict = []
        t0 = time.perf_counter()
        if which == "a":
            per_box_loop(dets, shapes, paths, folder, jdict, class_map)
        else:
            outputs.save_txt_batched(rows, (counts_t, counts), shapes, paths, folder, save_conf=True)
            outputs.save_json_batched(rows, (counts_t, counts), paths, jdict, class_map)
        return time.perf_counter() - t0, jdict

    ta, tb = [], []
    with tempfile.TemporaryDirectory() as tmp:
        tmp = Path(tmp)
        for r in range(a.rounds + 1):   # round 0: warm-up
            fa, fb = tmp / f"a{r}", tmp / f"b{r}"
            fa.mkdir()
            x, y = run("a", fa), run("b", fb)
            if r:
                ta.append(x[0]); tb.append(y[0])
        same_files = {f.name: f.read_bytes() for f in fa.iterdir()} == {f.name: f.read_bytes() for f in fb.iterdir()}
        same_json = x[1] == y[1]
    lines = [f"val_outputs_ab: bs {a.bs}, {sum(counts)} rows after NMS (conf 0.001, IoU 0.6, max_det 300), --save-txt --save-conf --save-json, {a.rounds} interleaved rounds after one warm-up",
             f"device: {torch.cuda.get_device_name(0)}   host CPU: {cpu_model()}",
             "(a) per-image, per-box loop (val.py's form):            " + "  ".join(f"{t * 1e3:9.2f}" for t in ta) + f"   median {statistics.median(ta) * 1e3:.2f} ms",
             "(b) save_txt_batched + save_json_batched (1 launch each): " + "  ".join(f"{t * 1e3:9.2f}" for t in tb) + f"   median {statistics.median(tb) * 1e3:.2f} ms",
             f"(b) below (a) in every round: {all(q < p for p, q in zip(ta, tb))}   files byte-equal: {same_files}   jdict equal: {same_json}"]
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text)


if __name__ == "__main__":
    main()
