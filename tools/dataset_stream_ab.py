"""A/B of one epoch of the train-mode loader on one MI355X with the image set in HBM and with it in pinned host memory (store="host": csrc/dataset_stage.hip through
yolov3_amd/dataset.py), in interleaved rounds.  Synthetic set: --images seeded images whose long side is --imgsz, --labels-per-image labels each; batches of --batch,
the augmentation values of data/hyps/hyp.scratch-low.yaml (or --hyp wild: rotation, shear, scale 0.9, mixup 0.3: up to eight images per item).  Three arms:

  resident           DeviceTrainDataset as it always was: the whole set in one HBM arena
  host, prefetch=0   the set in pinned host memory; the images of a batch are staged inside get_batch, on the stream of the launches
  host, prefetch=1   the images of batch k + 1 are staged on a side stream when batch k is handed out

Every round runs one epoch per arm from the same seed, the arms alternate, and every batch of the two host arms must equal the resident arm's: images byte for
byte, targets bit for bit.  Reported: the wall clock per batch of each arm (median over the rounds; an epoch ends in a synchronise), and, apart and by device events,
the stage launch of one batch -- its bytes, milliseconds and GB/s -- beside ONE contiguous pinned -> device copy_ of the same byte count in the same run: the copy
engine at its best, the yardstick and not a gate.  The one condition: the stage of a batch must take less than the train step it hides under (bench.py --mode train
--batch 64 on the same machine; pass its milliseconds as --step-ms).  With --step-ms the epochs are also run with that much device work between two batches (a
spinning kernel stands for the step), which is what prefetch=1 is for: the stage then runs under the step -- once with a loop that goes straight on to the next
batch (the host runs ahead of the device) and once with a step that ends in a host synchronise, as a loop that reads its loss every step does.  The report records what was measured.  One time limit:

    timeout -k 10 600 python tools/dataset_stream_ab.py [--images 512] [--imgsz 640] [--batch 64] [--rounds 3] [--hyp low] [--step-ms 55.5] [--out profiles/dataset_stream_ab.txt]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=512)
    ap.add_argument("--imgsz", type=int, default=640)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--labels-per-image", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--hyp", default="low", choices=["low", "wild"])
    ap.add_argument("--step-ms", type=float, default=0.0, help="the train step of the same batch size on the same machine (bench.py --mode train): the time a stage may take")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "dataset_stream_ab.txt"), help="the report is also written to this file ('' for none)")
    args = ap.parse_args()

    from yolov3_amd import DeviceTrainDataset, dataset, ops   # noqa: E402

    assert torch.cuda.is_available(), "dataset_stream_ab.py measures on an MI355X; there is nothing to measure without one"
    dev = torch.device("cuda:0")
    rs = np.random.RandomState(0)
    n, S, bs = args.images, args.imgsz, args.batch
    ar = np.exp(rs.normal(0.0, 0.35, n)).clip(0.4, 2.5)   # h / w
    hw = [(S, max(16, round(S / a))) if a > 1 else (max(16, round(S * a)), S) for a in ar]
    images = [rs.randint(0, 256, (h, w, 3), dtype=np.uint8) for h, w in hw]
    labels = [np.concatenate([rs.randint(0, 80, (m, 1)).astype(np.float64), rs.uniform(0.1, 0.9, (m, 2)), rs.uniform(0.02, 0.5, (m, 2))], 1).astype(np.float32)
              for m in rs.poisson(args.labels_per_image, n)]
    hyp = dict(ac.CASES[args.hyp]["hyp"])
    arms, build = {}, {}
    for name, kw in (("resident", {}), ("host, prefetch=0", dict(store="host", prefetch=0)), ("host, prefetch=1", dict(store="host", prefetch=1))):
        t0 = time.perf_counter()
        arms[name] = DeviceTrainDataset(images, labels, hyp, img_size=S, batch_size=bs, device=dev, **kw)
        torch.cuda.synchronize()
        build[name] = time.perf_counter() - t0
    nb = len(arms["resident"])

    def epoch(ds, seed, spin_ms=0.0, sync=False):
        """-> (wall seconds per batch, the batches: images and targets kept on the device)"""
        random.seed(seed)
        np.random.seed(seed)
        torch.cuda.synchronize()
        got, t = [], time.perf_counter()
        for im, targets, _, _ in ds:
            got.append((im, targets))
            if spin_ms:
                torch.cuda._sleep(int(spin_ms * 1e-3 * cycles_per_s))   # the step of this batch: device work on the current stream, the host runs on
                if sync:
                    torch.cuda.current_stream().synchronize()   # ... unless the loop reads something back every step
        torch.cuda.synchronize()
        return (time.perf_counter() - t) / nb, got

    cycles_per_s = 0.0
    if args.step_ms:   # calibrate the spinning kernel once: cycles per second of its counter
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda._sleep(1_000_000)
        e0.record()
        torch.cuda._sleep(20_000_000)
        e1.record()
        torch.cuda.synchronize()
        cycles_per_s = 20_000_000 / (e0.elapsed_time(e1) * 1e-3)

    for ds in arms.values():   # untimed: library load, allocator, the pinned buffers' first use
        epoch(ds, 99)
    wall = {name: [] for name in arms}
    under = {name: [] for name in arms}
    under_sync = {name: [] for name in arms}
    agree = True
    for r in range(args.rounds):
        ref = None
        for name, ds in arms.items():
            w, got = epoch(ds, r)
            wall[name].append(w)
            if ref is None:
                ref = got
            else:
                agree = agree and len(got) == len(ref) and all(torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32)) for a, b in zip(got, ref))
            del got
        del ref
        if args.step_ms:
            for name, ds in arms.items():
                under[name].append(epoch(ds, r, args.step_ms)[0])
            for name, ds in arms.items():
                under_sync[name].append(epoch(ds, r, args.step_ms, sync=True)[0])

    # the stage of one batch alone, and the contiguous copy of as many bytes
    ds = arms["host, prefetch=0"]
    st = ds._store
    random.seed(0)
    np.random.seed(0)
    stage_ms, copy_ms, nbytes, counts = [], [], [], []
    flat = torch.empty(st.half_bytes, dtype=torch.uint8, device=dev)
    for k in range(min(nb, 8)):
        needs = ds._needs(ds.draw_batch(k))
        unique, offsets = dataset.plan_slots(needs, st.slots, st.half_bytes)
        jobs = dataset.stage_jobs(unique, offsets, st.slots, st.chunk)
        jobs_dev = torch.from_numpy(jobs).to(dev)
        size = int(st.slots[unique].sum())
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        torch.cuda.synchronize()
        ev[0].record()
        ops.dataset_stage(st.arena, st.src, st.n, jobs_dev, len(unique), int(jobs[-1, 2]), st.halves[0], st.records[0], st.status)
        ev[1].record()
        torch.cuda.synchronize()
        ev[2].record()
        flat[:size].copy_(st.arena[:size], non_blocking=True)
        ev[3].record()
        torch.cuda.synchronize()
        if k:   # (the first launch loads the kernel)
            stage_ms.append(ev[0].elapsed_time(ev[1]))
            copy_ms.append(ev[2].elapsed_time(ev[3]))
            nbytes.append(size)
            counts.append(len(unique))
    st.check()

    med = statistics.median
    lines = [f"dataset stream A/B: {n} cached images (long side {S}, {arms['resident']._arena.numel() / 1e9:.2f} GB), batches of {bs}, hyp {args.hyp}, {nb} batches per epoch, "
             f"{args.rounds} interleaved rounds of one epoch per arm, {torch.cuda.get_device_name(0)}",
             f"device memory for the images: resident {arms['resident']._arena.numel() / 1e6:.1f} MB; host store {ds.ring_bytes / 1e6:.1f} MB (a ring of two halves of "
             f"{st.half_bytes / 1e6:.1f} MB, the worst batch) + {2 * 32 * n / 1e3:.1f} KB of record tables, beside {ds.host_bytes / 1e6:.1f} MB of pinned host memory",
             "building the set: " + ", ".join(f"{name} {build[name] * 1e3:.0f} ms" for name in arms)]
    for name in arms:
        lines.append(f"{name:<18} wall clock per batch (draws, pack, copy, stage, launches, offsets read): {med(wall[name]) * 1e3:8.3f} ms   "
                     f"(rounds: {', '.join(f'{w * 1e3:.3f}' for w in wall[name])})")
    if args.step_ms:
        for name in arms:
            lines.append(f"{name:<18} the same with {args.step_ms:.1f} ms of device work after every batch:               {med(under[name]) * 1e3:8.3f} ms   "
                         f"(over the work: {(med(under[name]) * 1e3 - args.step_ms):+.3f} ms)")
        for name in arms:
            lines.append(f"{name:<18} the same, the host synchronising after the work of every batch:            {med(under_sync[name]) * 1e3:8.3f} ms   "
                         f"(over the work: {(med(under_sync[name]) * 1e3 - args.step_ms):+.3f} ms)")
    gbs = [b / ms / 1e6 for b, ms in zip(nbytes, stage_ms)]
    cgbs = [b / ms / 1e6 for b, ms in zip(nbytes, copy_ms)]
    lines += [f"y3_dataset_stage alone (device events), {len(stage_ms)} batches of {med(counts):.0f} unique images, {med(nbytes) / 1e6:.1f} MB: {med(stage_ms):8.3f} ms   "
              f"{med(gbs):.1f} GB/s (min {min(gbs):.1f}, max {max(gbs):.1f})",
              f"one contiguous pinned -> device copy_ of the same bytes, same run (the yardstick):               {med(copy_ms):8.3f} ms   {med(cgbs):.1f} GB/s   "
              f"stage / copy rate {med(gbs) / med(cgbs):.2f}; the link's spec is 63 GB/s",
              f"agreement: every batch of both host arms equals the resident arm's, images byte for byte and targets bit for bit: {bool(agree)}"]
    if args.step_ms:
        ok = med(stage_ms) < args.step_ms
        lines.append(f"the condition: the stage of a batch ({med(stage_ms):.3f} ms) takes {'less' if ok else 'MORE'} than the {args.step_ms:.1f} ms train step of batch {bs} it hides under: "
                     f"{'met' if ok else 'NOT MET'} ({med(stage_ms) / args.step_ms * 100:.1f} % of the step)")
    report = "\n".join(lines)
    print(report)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(report + "\n")
    assert agree, "a host arm's batch differs from the resident arm's"


if __name__ == "__main__":
    main()
