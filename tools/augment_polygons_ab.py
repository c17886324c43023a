"""A/B of the polygon label path of one train-mode batch on one MI355X, in interleaved rounds: y3_augment_polygons + y3_augment_targets_polygons (csrc/augment.hip
through yolov3_amd/augment.py) against the NumPy statement of tests/augment_polygon_cases.py on the host, from the SAME draws.  Synthetic set: --images seeded images
whose long side is --imgsz, about --labels-per-image labels each, every label a polygon of 20 to 200 vertices inside its box (the labels are segments2boxes of the
polygons, as the reference's parser derives them); batches of --batch, the augmentation values of data/hyps/hyp.scratch-low.yaml.

  device   the polygon launch alone and the polygon form of the targets alone (device events), and the whole batch (wall clock, synchronised) of the polygon set
           and of the same set without its polygons; the host's one-time packing of the vertex table
  host     the labels of the same items through the statement (resample, transform, segment2box, box_candidates per label), one process
  parent   with --parent-lib (a libyolov3_hip.so built from the parent commit): the two launches of a box-only batch through this commit's library and through the
           parent's, loaded side by side and alternated in the same run (the order of the arms reversed every other round); the spread over the rounds of one
           library is the noise of that comparison

The device targets and fp64 boxes must equal the statement's bit for bit before anything is timed.  No speed-up is promised: the report records what was measured.

    timeout -k 10 600 python tools/augment_polygons_ab.py [--images 512] [--imgsz 640] [--batch 64] [--rounds 6] [--step-ms 55] [--parent-lib PATH] [--out profiles/augment_polygons_ab.txt]
"""
import argparse
import ctypes
import random
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import augment_cases as ac  # noqa: E402
import augment_polygon_cases as apc  # noqa: E402


def synthetic_set(n, S, per_image, rs):
    ar = np.exp(rs.normal(0.0, 0.35, n)).clip(0.4, 2.5)   # h / w
    hw = [(S, max(16, round(S / a))) if a > 1 else (max(16, round(S * a)), S) for a in ar]
    images = [rs.randint(0, 256, (h, w, 3), dtype=np.uint8) for h, w in hw]
    labels, segments = [], []
    for m in rs.poisson(per_image, n):
        polys = []
        for _ in range(m):
            (xc, yc), (bw, bh), k = rs.uniform(0.1, 0.9, 2), rs.uniform(0.02, 0.5, 2), int(rs.randint(20, 201))
            ang, rad = np.sort(rs.uniform(0, 2 * np.pi, k)), rs.uniform(0.45, 1.0, k)
            polys.append(np.clip(np.stack([xc + bw / 2 * rad * np.cos(ang), yc + bh / 2 * rad * np.sin(ang)], 1), 0.0, 1.0).astype(np.float32))
        segments.append(polys)
        labels.append(np.concatenate([rs.randint(0, 80, (m, 1)).astype(np.float32), apc.segments2boxes(polys)], 1).astype(np.float32) if m else np.zeros((0, 5), dtype=np.float32))
    return images, labels, segments, hw


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=512)
    ap.add_argument("--imgsz", type=int, default=640)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--labels-per-image", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--launches", type=int, default=20, help="launches timed per round and arm")
    ap.add_argument("--step-ms", type=float, default=0.0, help="the train step of the same batch size on the same machine (bench.py --mode train), for the share")
    ap.add_argument("--parent-lib", default="", help="libyolov3_hip.so of the parent commit: the box-only launches are compared with it")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "augment_polygons_ab.txt"), help="the report is also written to this file ('' for none)")
    args = ap.parse_args()

    from yolov3_amd import DeviceTrainDataset, _lib, augment, ops   # noqa: E402

    assert torch.cuda.is_available(), "augment_polygons_ab.py measures on an MI355X; there is nothing to measure without one"
    dev = torch.device("cuda:0")
    n, S, bs = args.images, args.imgsz, args.batch
    images, labels, segments, hw = synthetic_set(n, S, args.labels_per_image, np.random.RandomState(0))
    hyp = dict(ac.CASES["low"]["hyp"])
    t0 = time.perf_counter()
    vertices, _ = augment.pack_polygons(labels, segments)
    t_pack = time.perf_counter() - t0
    ds = DeviceTrainDataset(images, labels, hyp, img_size=S, batch_size=bs, device=dev, segments=segments)
    box = DeviceTrainDataset(images, labels, hyp, img_size=S, batch_size=bs, device=dev)
    random.seed(0)
    np.random.seed(0)
    med = statistics.median

    def events(fn, count):
        """milliseconds per call of `count` calls of fn, by device events"""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(count):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / count

    def wall(d, k, items):
        torch.cuda.synchronize()
        t = time.perf_counter()
        d.get_batch(k, items=items)
        torch.cuda.synchronize()
        return time.perf_counter() - t

    # equal first
    items = ds.draw_batch(0)
    upper = int(sum(len(labels[j]) for it in items for mo in it.mosaics for j in mo.indices))
    st = apc.batch_statement(items, labels, segments, hw, S)
    _, targets, _, _ = ds.get_batch(0, items=items)
    boxes, inside, words = (t.cpu().numpy() for t in ds.polygons)
    w = st["written"]
    agree = (np.array_equal(targets.cpu().numpy().view(np.int32), st["targets"].view(np.int32)) and np.array_equal(boxes[w].view(np.int64), st["boxes"][w].view(np.int64))
             and np.array_equal(inside[w], st["inside"][w]) and np.array_equal(words, st["words"]))
    assert agree, "the device and the statement differ: nothing is timed"
    rec = torch.from_numpy(augment.pack_items(items).view(np.uint8).copy()).to(dev)
    out = torch.empty((len(items), 3, S, S), dtype=torch.uint8, device=dev)

    def polygons():
        return ops.augment_polygons(ds._vertices, ds._vertex_offsets, ds._label_offsets, ds._records, ds.n, rec, len(items), S, upper)

    ws = polygons()
    arms = {
        "y3_augment_polygons": polygons,
        "y3_augment_targets_polygons": lambda: ops.augment_targets_polygons(ds._labels, ds._label_offsets, ds._records, ds.n, rec, len(items), S, upper, *ws),
        "y3_augment_targets": lambda: ops.augment_targets(box._labels, box._label_offsets, box._records, box.n, rec, len(items), S, upper),
        "y3_augment_batch": lambda: ops.augment_batch(box._arena, box._records, box.n, rec, len(items), S, torch.uint8, out),
    }
    parent = None
    if args.parent_lib:   # the parent's two exports under the header's own argument types, next to this commit's library
        parent = ctypes.CDLL(args.parent_lib)
        for name in ("y3_augment_batch", "y3_augment_targets"):
            getattr(parent, name).restype, getattr(parent, name).argtypes = _lib._SIGNATURES[name]
        tg, of = torch.empty(upper, 6, dtype=torch.float32, device=dev), torch.empty(len(items) + 1, dtype=torch.int64, device=dev)
        arms["parent y3_augment_targets"] = lambda: parent.y3_augment_targets(box._labels.data_ptr(), box._label_offsets.data_ptr(), box._records.data_ptr(), box.n, rec.data_ptr(),
                                                                              len(items), S, tg.data_ptr(), upper, of.data_ptr(), ops.stream_ptr())
        arms["parent y3_augment_batch"] = lambda: parent.y3_augment_batch(box._arena.data_ptr(), box._arena.numel(), box._records.data_ptr(), box.n, rec.data_ptr(), len(items),
                                                                          out.data_ptr(), 3, S, ops.stream_ptr())
        assert arms["parent y3_augment_targets"]() == 0 and arms["parent y3_augment_batch"]() == 0
        mine = ops.augment_targets(box._labels, box._label_offsets, box._records, box.n, rec, len(items), S, upper)
        nl = int(of.cpu()[-1])
        assert torch.equal(mine[1], of) and torch.equal(mine[0][:nl], tg[:nl]), "the box-only targets differ from the parent's"
    for fn in arms.values():   # untimed
        fn()
    wall(ds, 0, items), wall(box, 0, items)
    times = {k: [] for k in arms}
    walls, host = {"polygon set": [], "box-only set": []}, []
    for r in range(args.rounds):
        for name, fn in (list(arms.items())[::-1] if r % 2 else arms.items()):   # the arms in turn, the order reversed every other round
            times[name].append(events(fn, args.launches))
        walls["polygon set"].append(wall(ds, 0, items))
        walls["box-only set"].append(wall(box, 0, items))
        t = time.perf_counter()
        apc.batch_statement(items, labels, segments, hw, S)
        host.append(time.perf_counter() - t)
    lines = [f"augment polygons A/B: {n} cached images (long side {S}), {sum(len(l) for l in labels)} labels, {len(vertices)} vertices (20 .. 200 per polygon), batches of {bs}, "
             f"hyp low, {args.rounds} interleaved rounds of {args.launches} launches per arm, {torch.cuda.get_device_name(0)}",
             f"the batch: {upper} label rows in its tiles, {len(targets)} survivors, {int((words == 1).sum())} of {int(sum(len(it.mosaics) for it in items))} mosaics on the polygon path",
             f"agreement: device targets, fp64 boxes and path words equal the statement bit for bit {bool(agree)}",
             f"host, once per set: packing the vertex table {t_pack * 1e3:.1f} ms"]
    for name, v in times.items():
        lines.append(f"  {name:34s} {med(v) * 1e3:9.1f} us   (rounds {min(v) * 1e3:.1f} .. {max(v) * 1e3:.1f})")
    for name, v in walls.items():
        lines.append(f"device batch of the {name:13s} wall clock, synchronised, packed items given: {med(v) * 1e3:9.3f} ms   (rounds {min(v) * 1e3:.3f} .. {max(v) * 1e3:.3f})")
    new = med(times["y3_augment_polygons"]) + med(times["y3_augment_targets_polygons"]) - med(times["y3_augment_targets"])
    lines.append(f"host statement, labels only (NumPy, one process): {med(host) * 1e3:9.1f} ms   host / (polygon launch + polygon targets) "
                 f"{med(host) * 1e3 / (med(times['y3_augment_polygons']) + med(times['y3_augment_targets_polygons'])):.0f}")
    lines.append(f"added per batch by polygon labels (polygon launch + polygon targets - box targets): {new * 1e3:.1f} us")
    if parent is not None:
        for name in ("y3_augment_batch", "y3_augment_targets"):
            a, b = times[name], times["parent " + name]
            lines.append(f"box-only {name}: this commit {med(a) * 1e3:.1f} us, parent {med(b) * 1e3:.1f} us, difference {(med(a) - med(b)) * 1e3:+.1f} us; "
                         f"noise (spread of one library's rounds) {max(max(a) - min(a), max(b) - min(b)) * 1e3:.1f} us")
    if args.step_ms:
        lines.append(f"share of a {args.step_ms:.1f} ms train step of batch {bs}: the polygon launch {med(times['y3_augment_polygons']) / args.step_ms * 100:.2f} %, "
                     f"all that polygons add {new / args.step_ms * 100:.2f} %")
    report = "\n".join(lines)
    print(report)
    if args.out:
        Path(args.out).write_text(report + "\n")


if __name__ == "__main__":
    main()
