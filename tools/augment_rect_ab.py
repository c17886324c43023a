"""A/B of the two square launches of one train-mode batch on one MI355X after csrc/augment.hip went from S x S to H x W items: y3_augment_batch and y3_augment_targets
through this tree's library against the PARENT commit's library (--parent-lib, a libyolov3_hip.so built from a clean export of the parent), both loaded in the same
process and alternated in interleaved rounds, the order of the arms reversed every other round.  The spread over the rounds of the parent's own arm is the noise of the
comparison.  Synthetic set as in tools/augment_polygons_ab.py: --images seeded images whose long side is --imgsz, about --labels-per-image labels each, batches of
--batch, the augmentation values of data/hyps/hyp.scratch-low.yaml (mosaic items).

Also, for the record, one rect batch: --batch items letterboxed to --rect-shape (H W, default 448 640 -- 640 wide, 448 high) through y3_augment_batch_hw and
y3_augment_targets_hw, from a DeviceRectTrainDataset over seeded images that touch that shape.

Both libraries must write identical bytes before anything is timed, and both are called the same way (the C export itself, into buffers allocated once).  Acceptance
as the report states it, per launch and for the two together: the new median exceeds the parent's by no more than the parent's own round-to-round spread in that run.

    timeout -k 10 600 python tools/augment_rect_ab.py --parent-lib PATH [--images 512] [--imgsz 640] [--batch 64] [--rounds 8] [--launches 20] [--out profiles/augment_rect_ab.txt]
"""
import argparse
import ctypes
import random
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import augment_cases as ac  # noqa: E402


def synthetic_set(n, S, per_image, rs):
    ar = np.exp(rs.normal(0.0, 0.35, n)).clip(0.4, 2.5)   # h / w
    hw = [(S, max(16, round(S / a))) if a > 1 else (max(16, round(S * a)), S) for a in ar]
    images = [rs.randint(0, 256, (h, w, 3), dtype=np.uint8) for h, w in hw]
    labels = []
    for m in rs.poisson(per_image, n):
        wh = rs.uniform(0.02, 0.5, (m, 2))
        c = rs.uniform(0.0, 1.0, (m, 2)) * (1 - wh) + wh / 2
        labels.append(np.concatenate([rs.randint(0, 80, (m, 1)).astype(np.float64), c, wh], 1).astype(np.float32).reshape(-1, 5))
    return images, labels


def rect_set(n, H, W, per_image, rs):
    """wide images that touch the H x W batch shape: the width is W, the height at most H (r = 1)"""
    images = [rs.randint(0, 256, (int(h), W, 3), dtype=np.uint8) for h in np.concatenate([[H], rs.randint(H - 31, H + 1, n - 1)])]
    labels = []
    for m in rs.poisson(per_image, n):
        wh = rs.uniform(0.02, 0.5, (m, 2))
        c = rs.uniform(0.0, 1.0, (m, 2)) * (1 - wh) + wh / 2
        labels.append(np.concatenate([rs.randint(0, 80, (m, 1)).astype(np.float64), c, wh], 1).astype(np.float32).reshape(-1, 5))
    return images, labels


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=512)
    ap.add_argument("--imgsz", type=int, default=640)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--labels-per-image", type=int, default=7)
    ap.add_argument("--rect-shape", type=int, nargs=2, default=(448, 640), metavar=("H", "W"))
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--launches", type=int, default=20, help="launches timed per round and arm")
    ap.add_argument("--parent-lib", required=True, help="libyolov3_hip.so of the parent commit")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "augment_rect_ab.txt"), help="the report is also written to this file ('' for none)")
    args = ap.parse_args()

    from yolov3_amd import DeviceRectTrainDataset, DeviceTrainDataset, _lib, augment, ops   # noqa: E402

    assert torch.cuda.is_available(), "augment_rect_ab.py measures on an MI355X; there is nothing to measure without one"
    dev = torch.device("cuda:0")
    n, S, bs = args.images, args.imgsz, args.batch
    hyp = dict(ac.CASES["low"]["hyp"])
    images, labels = synthetic_set(n, S, args.labels_per_image, np.random.RandomState(0))
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

    items = box.draw_batch(0)
    upper = int(sum(len(labels[j]) for it in items for mo in it.mosaics for j in mo.indices))
    rec = torch.from_numpy(augment.pack_items(items).view(np.uint8).copy()).to(dev)
    parent = ctypes.CDLL(args.parent_lib)   # the parent's two exports under the header's own argument types, next to this tree's library
    for name in ("y3_augment_batch", "y3_augment_targets"):
        getattr(parent, name).restype, getattr(parent, name).argtypes = _lib._SIGNATURES[name]
    # both libraries are called the same way -- the C export itself, into buffers allocated once -- so that the host's share of a 36 us launch is the same in both arms
    arms, bufs = {}, {}
    for who, lib in (("", _lib.lib()), ("parent ", parent)):
        out = torch.empty((len(items), 3, S, S), dtype=torch.uint8, device=dev)
        tg, of = torch.zeros(upper, 6, dtype=torch.float32, device=dev), torch.zeros(len(items) + 1, dtype=torch.int64, device=dev)
        bufs[who] = (out, tg, of)
        arms[who + "y3_augment_batch"] = lambda lib=lib, out=out: lib.y3_augment_batch(box._arena.data_ptr(), box._arena.numel(), box._records.data_ptr(), box.n, rec.data_ptr(), len(items),
                                                                                       out.data_ptr(), 3, S, ops.stream_ptr())
        arms[who + "y3_augment_targets"] = lambda lib=lib, tg=tg, of=of: lib.y3_augment_targets(box._labels.data_ptr(), box._label_offsets.data_ptr(), box._records.data_ptr(), box.n,
                                                                                                rec.data_ptr(), len(items), S, tg.data_ptr(), upper, of.data_ptr(), ops.stream_ptr())
    arms = {k: arms[k] for k in ("y3_augment_batch", "parent y3_augment_batch", "y3_augment_targets", "parent y3_augment_targets")}
    # equal first
    assert all(fn() == 0 for fn in arms.values())
    torch.cuda.synchronize()
    (out, tg, of), (out_p, tg_p, of_p) = bufs[""], bufs["parent "]
    nl = int(of.cpu()[-1])
    agree = bool(torch.equal(out, out_p) and torch.equal(of, of_p) and torch.equal(tg[:nl], tg_p[:nl]))
    assert agree, "this tree's square batch differs from the parent's: nothing is timed"

    # the rect batch, for the record
    H, W = args.rect_shape
    r_images, r_labels = rect_set(bs, H, W, args.labels_per_image, np.random.RandomState(1))
    rds = DeviceRectTrainDataset(r_images, r_labels, hyp, img_size=max(H, W), batch_size=bs, stride=32, device=dev)
    assert [tuple(int(v) for v in s) for s in rds.batch_shapes] == [(H, W)], rds.batch_shapes
    r_items = rds.draw_batch(0)
    r_upper = int(sum(len(rds.labels[it.index]) for it in r_items))
    r_rec = torch.from_numpy(augment.pack_items(r_items).view(np.uint8).copy()).to(dev)
    r_out = torch.empty((len(r_items), 3, H, W), dtype=torch.uint8, device=dev)
    rect_arms = {
        "y3_augment_batch_hw": lambda: ops.augment_batch_hw(rds._arena, rds._records, rds.n, r_rec, len(r_items), H, W, torch.uint8, r_out),
        "y3_augment_targets_hw": lambda: ops.augment_targets_hw(rds._labels, rds._label_offsets, rds._records, rds.n, r_rec, len(r_items), H, W, r_upper),
    }
    for fn in list(arms.values()) + list(rect_arms.values()):   # untimed
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in list(arms) + list(rect_arms)}
    for r in range(args.rounds):
        for name, fn in (list(arms.items())[::-1] if r % 2 else arms.items()):   # the arms in turn, the order reversed every other round
            times[name].append(events(fn, args.launches))
        for name, fn in rect_arms.items():
            times[name].append(events(fn, args.launches))
    lines = [f"augment rect A/B: {n} cached images (long side {S}), {sum(len(l) for l in labels)} labels, batches of {bs}, hyp low, {args.rounds} interleaved rounds of {args.launches} "
             f"launches per arm, {torch.cuda.get_device_name(0)}",
             f"the square batch: {len(items)} mosaic items at {S}x{S}, {upper} label rows in its tiles, {nl} survivors",
             f"agreement: this tree's images, targets and offsets equal the parent library's byte for byte {agree}"]
    for name, v in times.items():
        lines.append(f"  {name:28s} {med(v) * 1e3:9.1f} us   (rounds {min(v) * 1e3:.1f} .. {max(v) * 1e3:.1f})")
    for name in ("y3_augment_batch", "y3_augment_targets"):
        a, b = times[name], times["parent " + name]
        diff, spread = (med(a) - med(b)) * 1e3, (max(b) - min(b)) * 1e3
        lines.append(f"square {name}: this tree {med(a) * 1e3:.1f} us, parent {med(b) * 1e3:.1f} us, difference {diff:+.1f} us; the parent's own round-to-round spread {spread:.1f} us; "
                     f"within it: {diff <= spread}")
    both = [x + y for x, y in zip(times["y3_augment_batch"], times["y3_augment_targets"])], [x + y for x, y in zip(times["parent y3_augment_batch"], times["parent y3_augment_targets"])]
    diff, spread = (med(both[0]) - med(both[1])) * 1e3, (max(both[1]) - min(both[1])) * 1e3
    lines.append(f"the square batch, both launches: this tree {med(both[0]) * 1e3:.1f} us, parent {med(both[1]) * 1e3:.1f} us, difference {diff:+.1f} us; the parent's own round-to-round "
                 f"spread {spread:.1f} us; within it: {diff <= spread}")
    lines.append(f"one rect batch, for the record: {len(r_items)} letterbox items at {H}x{W} (H x W), {r_upper} label rows: y3_augment_batch_hw {med(times['y3_augment_batch_hw']) * 1e3:.1f} us, "
                 f"y3_augment_targets_hw {med(times['y3_augment_targets_hw']) * 1e3:.1f} us")
    report = "\n".join(lines)
    print(report)
    if args.out:
        Path(args.out).write_text(report + "\n")


if __name__ == "__main__":
    main()
