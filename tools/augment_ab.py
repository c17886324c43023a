"""A/B of one train-mode batch on one MI355X, in interleaved rounds: DeviceTrainDataset (csrc/augment.hip through yolov3_amd/augment.py) against the same batch made
on the host, in one process, by the NumPy statements of tests/augment_cases.py (the canvas pasted, warp_affine_u8, the mixup blend, bgr2hsv_u8 / the tables /
hsv2bgr_u8, the flips, CHW RGB) from the SAME draws.  Synthetic set: --images seeded images whose long side is --imgsz, --labels-per-image labels each; batches of
--batch, the augmentation values of data/hyps/hyp.scratch-low.yaml (or --hyp wild: rotation, shear, scale 0.9, mixup 0.3).

  device batch   draw_item for every item, pack, the one host -> device copy, y3_augment_batch, y3_augment_targets, the read of the bs + 1 offsets (wall clock,
                 synchronised) -- and, apart, the host's share of it (draw + pack) and the two launches alone (device events)
  host batch     the images of the same items through the NumPy statements (the labels are left out: a few hundred rows per batch)

Every round times each arm once on its own batch, the arms alternate; medians over the rounds are printed, and the device batch must equal the host batch byte for
byte.  The figure to read is the device time per batch as a share of the batch's train step (bench.py --mode train --batch 64 on the same machine; pass its
milliseconds as --step-ms to have the share printed).  No speed-up is promised: the report records what was measured.  Run under one time limit:

    timeout -k 10 600 python tools/augment_ab.py [--images 512] [--imgsz 640] [--batch 64] [--rounds 3] [--hyp low] [--step-ms 55] [--out profiles/augment_ab.txt]
"""
import argparse
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


def host_batch(items, images, s):
    """the images of `items` by the NumPy statements -> uint8 (bs, 3, s, s)"""
    out = []
    for it in items:
        warped = []
        for mo in it.mosaics:
            canvas = np.full((mo.canvas, mo.canvas, 3), 114, dtype=np.uint8)
            for j, (x1a, y1a, x2a, y2a, x1b, y1b, x2b, y2b) in zip(mo.indices, mo.rects):
                canvas[y1a:y2a, x1a:x2a] = images[j][y1b:y2b, x1b:x2b]
            warped.append(ac.warp_affine_u8(canvas, mo.M[:2], (s, s)))
        im = warped[0] if it.ratio is None else (warped[0] * it.ratio + warped[1] * (1 - it.ratio)).astype(np.uint8)
        if it.luts is not None:
            hsv = ac.bgr2hsv_u8(im)
            im = ac.hsv2bgr_u8(np.stack([it.luts[c][hsv[..., c]] for c in range(3)], -1))
        if it.flipud:
            im = np.flipud(im)
        if it.fliplr:
            im = np.fliplr(im)
        out.append(np.ascontiguousarray(im.transpose((2, 0, 1))[::-1]))
    return torch.from_numpy(np.stack(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=512)
    ap.add_argument("--imgsz", type=int, default=640)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--labels-per-image", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--device-batches", type=int, default=8, help="device batches timed per round (the host arm makes one)")
    ap.add_argument("--hyp", default="low", choices=["low", "wild"])
    ap.add_argument("--step-ms", type=float, default=0.0, help="the train step of the same batch size on the same machine (bench.py --mode train), for the share")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "augment_ab.txt"), help="the report is also written to this file ('' for none)")
    args = ap.parse_args()

    from yolov3_amd import DeviceTrainDataset, augment, ops   # noqa: E402

    assert torch.cuda.is_available(), "augment_ab.py measures on an MI355X; there is nothing to measure without one"
    dev = torch.device("cuda:0")
    rs = np.random.RandomState(0)
    n, S, bs = args.images, args.imgsz, args.batch
    ar = np.exp(rs.normal(0.0, 0.35, n)).clip(0.4, 2.5)   # h / w
    hw = [(S, max(16, round(S / a))) if a > 1 else (max(16, round(S * a)), S) for a in ar]
    images = [rs.randint(0, 256, (h, w, 3), dtype=np.uint8) for h, w in hw]
    labels = [np.concatenate([rs.randint(0, 80, (m, 1)).astype(np.float64), rs.uniform(0.1, 0.9, (m, 2)), rs.uniform(0.02, 0.5, (m, 2))], 1).astype(np.float32)
              for m in rs.poisson(args.labels_per_image, n)]
    hyp = dict(ac.CASES[args.hyp]["hyp"])
    t0 = time.perf_counter()
    ds = DeviceTrainDataset(images, labels, hyp, img_size=S, batch_size=bs, device=dev)
    torch.cuda.synchronize()
    t_build = time.perf_counter() - t0
    random.seed(0)
    np.random.seed(0)
    nb = len(ds)

    def device_batches(count, first):
        """-> (wall seconds per batch, host seconds per batch (draw + pack), the last batch and its items)"""
        torch.cuda.synchronize()
        t_host, t = 0.0, time.perf_counter()
        for k in range(first, first + count):
            th = time.perf_counter()
            items = ds.draw_batch(k % nb)
            augment.pack_items(items, ds._stage_rec[: len(items)])
            t_host += time.perf_counter() - th
            got = ds.get_batch(k % nb, items=items)
        torch.cuda.synchronize()
        return (time.perf_counter() - t) / count, t_host / count, got, items

    def launches(items):
        """the two launches alone, by device events: milliseconds (images, targets)"""
        rec = torch.from_numpy(augment.pack_items(items).view(np.uint8).copy()).to(dev)
        upper = int(sum(len(labels[j]) for it in items for mo in it.mosaics for j in mo.indices))
        out = torch.empty((len(items), 3, S, S), dtype=torch.uint8, device=dev)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        ev[0].record()
        ops.augment_batch(ds._arena, ds._records, ds.n, rec, len(items), S, torch.uint8, out)
        ev[1].record()
        ops.augment_targets(ds._labels, ds._label_offsets, ds._records, ds.n, rec, len(items), S, upper)
        ev[2].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]), ev[1].elapsed_time(ev[2])

    device_batches(2, 0)   # untimed: library load, allocator
    wall, host_share, k_im, k_tg, host_t, agree, rows = [], [], [], [], [], True, []
    k = 0
    for _ in range(args.rounds):
        w, h, (im, targets, _, _), items = device_batches(args.device_batches, k)
        k += args.device_batches
        wall.append(w)
        host_share.append(h)
        a, b = launches(items)
        k_im.append(a)
        k_tg.append(b)
        rows.append(len(targets))
        t = time.perf_counter()
        want = host_batch(items, images, S)
        host_t.append(time.perf_counter() - t)
        agree = agree and torch.equal(im.cpu(), want)
    med = statistics.median
    lines = [f"augment A/B: {n} cached images (long side {S}, {ds._arena.numel() / 1e9:.2f} GB), batches of {bs}, hyp {args.hyp}, {args.rounds} interleaved rounds of "
             f"{args.device_batches} device batches and 1 host batch, {torch.cuda.get_device_name(0)}",
             f"building the DeviceTrainDataset (upload through one pinned buffer): {t_build * 1e3:.0f} ms once",
             f"device batch, wall clock (draws, pack, copy, two launches, offsets read): {med(wall) * 1e3:9.3f} ms   ({bs / med(wall):.0f} img/s)",
             f"  of which the host's draws and packing:                               {med(host_share) * 1e3:9.3f} ms",
             f"  y3_augment_batch alone (device events):                              {med(k_im):9.3f} ms   ({bs * 3 * S * S / med(k_im) / 1e6:.1f} GB/s of output)",
             f"  y3_augment_targets alone (device events):                            {med(k_tg):9.3f} ms   ({med(rows):.0f} surviving rows)",
             f"host batch, images only (NumPy statements, one process):               {med(host_t) * 1e3:9.1f} ms   ({bs / med(host_t):.1f} img/s)   host / device {med(host_t) / med(wall):.0f}",
             f"agreement: every compared device batch equals the host batch byte for byte {bool(agree)}"]
    if args.step_ms:
        lines.append(f"share of a {args.step_ms:.1f} ms train step of batch {bs}: wall {med(wall) * 1e3 / args.step_ms * 100:.1f} %, the two launches {(med(k_im) + med(k_tg)) / args.step_ms * 100:.1f} %")
    report = "\n".join(lines)
    print(report)
    if args.out:
        Path(args.out).write_text(report + "\n")


if __name__ == "__main__":
    main()
