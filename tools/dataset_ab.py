"""A/B of one pass over a cached validation set at val2017 scale on one MI355X, in interleaved rounds: DeviceDataset (csrc/dataset.hip through
yolov3_amd/dataset.py) against a torch.utils.data.DataLoader over the SAME cached arrays -- the host form of the reference's augment=False loader
(utils/dataloaders.py:659-735, 825-830), written here with NumPy: np.pad with 114, transpose((2, 0, 1))[::-1], the two label conversions, collate_fn; --workers
worker processes, pinned memory, then .to(device).  Synthetic set: --images seeded images whose long side is --imgsz, aspect ratios spread like a photo collection,
--labels-per-image labels each; rect batches of --batch with pad 0.5.

  pass         every batch of one epoch on the device (images uint8 and targets), nothing else
  run_batches  val.run_batches end to end over the same feed (yolov3, half): forward, NMS, matching, AP

The workers are fresh processes (forkserver) that never open the GPU; the cached images reach them through shared memory, not through a copy.  They are sized by
the 16 CPUs a GPU job gets, not by os.cpu_count(), persist across the rounds, and one untimed epoch warms both feeds up.  Every round times each arm once, the arms
alternate within a round; medians over the rounds and the ratio host / device are printed.  No speed-up is promised: the report records what was measured.
Run on the GPU machine under one time limit:

    timeout -k 10 900 python tools/dataset_ab.py [--images 5000] [--imgsz 640] [--batch 32] [--workers 16] [--rounds 3] [--out profiles/dataset_ab.txt]
"""
import argparse
import shutil
import statistics
import sys
import tempfile
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


class HostSet(torch.utils.data.Dataset):
    """the host form over the cached arrays: `arena` a shared-memory uint8 tensor holding every (h, w, 3) image at offsets[i], rows = (h, w, H, W, top, left) per image"""

    def __init__(self, arena, offsets, rows, labels, paths, shapes):
        self.arena, self.offsets, self.rows, self.labels, self.paths, self.shapes = arena, offsets, rows, labels, paths, shapes

    def __len__(self):
        return len(self.rows)

    def __getitem__(self, i):
        h, w, H, W, top, left = self.rows[i]
        if isinstance(self.arena, str):   # (a path: mapped once per worker)
            self.arena = torch.from_numpy(np.memmap(self.arena, dtype=np.uint8, mode="r+"))
        img = self.arena[self.offsets[i] : self.offsets[i] + h * w * 3].numpy().reshape(h, w, 3)
        img = np.pad(img, ((top, H - h - top), (left, W - w - left), (0, 0)), mode="constant", constant_values=114)
        labels = self.labels[i].copy()
        if labels.size:
            x, padw, padh = labels[:, 1:], (W - w) / 2, (H - h) / 2
            xy = np.empty_like(x)
            xy[:, 0] = w * (x[:, 0] - x[:, 2] / 2) + padw
            xy[:, 1] = h * (x[:, 1] - x[:, 3] / 2) + padh
            xy[:, 2] = w * (x[:, 0] + x[:, 2] / 2) + padw
            xy[:, 3] = h * (x[:, 1] + x[:, 3] / 2) + padh
            xy[:, [0, 2]] = xy[:, [0, 2]].clip(0, W - 1e-3)
            xy[:, [1, 3]] = xy[:, [1, 3]].clip(0, H - 1e-3)
            labels[:, 1] = ((xy[:, 0] + xy[:, 2]) / 2) / W
            labels[:, 2] = ((xy[:, 1] + xy[:, 3]) / 2) / H
            labels[:, 3] = (xy[:, 2] - xy[:, 0]) / W
            labels[:, 4] = (xy[:, 3] - xy[:, 1]) / H
        out = torch.zeros((len(labels), 6))
        if len(labels):
            out[:, 1:] = torch.from_numpy(labels)
        return torch.from_numpy(np.ascontiguousarray(img.transpose((2, 0, 1))[::-1])), out, self.paths[i], self.shapes[i]


def collate_fn(batch):
    im, label, path, shapes = zip(*batch)
    for i, lb in enumerate(label):
        lb[:, 0] = i
    return torch.stack(im, 0), torch.cat(label, 0), path, shapes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=5000)
    ap.add_argument("--imgsz", type=int, default=640)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--labels-per-image", type=int, default=7)
    ap.add_argument("--workers", type=int, default=16, help="the CPUs a GPU job gets, not os.cpu_count()")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--model", default="yolov3.yaml")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "dataset_ab.txt"), help="the report is also written to this file ('' for none)")
    args = ap.parse_args()

    # the cached set, in one shared-memory arena (before the GPU is touched: the workers below are started from a fork server that never sees it)
    rs = np.random.RandomState(0)
    n, S = args.images, args.imgsz
    ar = np.exp(rs.normal(0.0, 0.35, n)).clip(0.4, 2.5)   # h / w
    hw = [(S, max(16, round(S / a))) if a > 1 else (max(16, round(S * a)), S) for a in ar]
    offsets = np.zeros(n + 1, dtype=np.int64)
    np.cumsum([-(-h * w * 3 // 16) * 16 for h, w in hw], out=offsets[1:])
    total, tmp = int(offsets[-1]), None
    if shutil.disk_usage("/dev/shm").free > total + (1 << 28):
        backing = "shared memory"
        arena = torch.empty(total, dtype=torch.uint8).share_memory_()
        flat = arena.numpy()
    else:   # a small /dev/shm: the page cache behind a temporary file serves the workers instead
        backing = "a memory-mapped temporary file"
        tmp = tempfile.NamedTemporaryFile(prefix="dataset_ab_", suffix=".u8")
        flat = np.memmap(tmp.name, dtype=np.uint8, mode="w+", shape=(total,))
        arena = tmp.name
    chunk = 1 << 26
    for a in range(0, len(flat), chunk):
        flat[a : a + chunk] = rs.randint(0, 256, min(chunk, len(flat) - a), dtype=np.uint8)
    images = [flat[offsets[i] : offsets[i] + h * w * 3].reshape(h, w, 3) for i, (h, w) in enumerate(hw)]
    labels = [np.concatenate([rs.randint(0, 80, (m, 1)).astype(np.float64), rs.uniform(0.1, 0.9, (m, 2)), rs.uniform(0.02, 0.5, (m, 2))], 1).astype(np.float32)
              for m in rs.poisson(args.labels_per_image, n)]
    paths = [f"val/{i:012d}.jpg" for i in range(n)]
    loader_args = dict(num_workers=args.workers, pin_memory=True, collate_fn=collate_fn, persistent_workers=True, multiprocessing_context="forkserver")

    from yolov3_amd import DetectionModel, DeviceDataset, dataset, run_batches   # noqa: E402

    assert torch.cuda.is_available(), "dataset_ab.py measures on an MI355X; there is nothing to measure without one"
    dev = torch.device("cuda:0")
    t0 = time.perf_counter()
    ds = DeviceDataset(images, labels, img_size=S, batch_size=args.batch, stride=32, pad=0.5, rect=True, paths=paths, device=dev)
    torch.cuda.synchronize()
    t_build = time.perf_counter() - t0
    lay = dataset.layout(hw, hw, S, args.batch, 32, 0.5, True)
    rows = [None] * n
    for j, i in enumerate(lay.order):
        H, W = (int(v) for v in lay.batch_shapes[lay.batch[j]])
        rows[i] = (hw[i][0], hw[i][1], H, W, int(lay.top[j]), int(lay.left[j]))
    host_shapes = [None] * n
    for j, i in enumerate(lay.order):
        host_shapes[i] = lay.shapes[j]
    order = [int(i) for i in lay.order]
    host = torch.utils.data.DataLoader(HostSet(arena, offsets.tolist(), rows, labels, paths, host_shapes),
                                       batch_sampler=[order[a : a + args.batch] for a in range(0, n, args.batch)], **loader_args)

    def host_feed():
        for im, targets, p, s in host:
            yield im.to(dev, non_blocking=True), targets.to(dev, non_blocking=True), p, s

    def consume(feed):
        k = 0
        for im, targets, _, _ in feed:
            k += im.shape[0]
        return k

    model = DetectionModel(args.model).to(dev).half().eval()

    def validate(feed):
        with torch.no_grad():
            return run_batches(model, feed, nc=80, half=True)[0]

    def timed(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t, r

    # one untimed epoch of both feeds: worker start-up, library load, allocator -- and the two feeds must agree
    agree = True
    for (a, ta, pa, sa), (b, tb, pb, sb) in zip(ds, host_feed()):
        agree = agree and torch.equal(a, b) and torch.equal(ta, tb) and pa == pb and sa == sb
    validate(ds.get_batch(k) for k in range(2))
    arms = {"pass": (lambda: consume(ds), lambda: consume(host_feed())), "run_batches": (lambda: validate(ds), lambda: validate(host_feed()))}
    times = {name: ([], []) for name in arms}
    results = {}
    for _ in range(args.rounds):
        for name, (d, h) in arms.items():
            td, rd = timed(d)
            th, rh = timed(h)
            times[name][0].append(td)
            times[name][1].append(th)
            results[name] = (rd, rh)
    del host   # (the persistent workers end with the loader)
    gb = float(offsets[-1]) / 1e9
    lines = [f"dataset A/B: {n} cached images (long side {S}, {gb:.2f} GB), {sum(len(l) for l in labels)} labels, {len(ds)} rect batches of {args.batch}, {args.rounds} interleaved rounds, "
             f"{torch.cuda.get_device_name(0)}, {args.workers} loader workers (forkserver, persistent, pinned memory; the cache in {backing}), model {args.model} fp16",
             f"building the DeviceDataset (layout, upload through one pinned buffer): {t_build * 1e3:.0f} ms once",
             f"{'arm':12s} {'device ms':>12s} {'host ms':>12s} {'host / device':>14s} {'device img/s':>13s} {'host img/s':>11s}"]
    for name, (td, th) in times.items():
        a, b = statistics.median(td), statistics.median(th)
        lines.append(f"{name:12s} {a * 1e3:12.1f} {b * 1e3:12.1f} {b / a:14.2f} {n / a:13.0f} {n / b:11.0f}")
    lines.append(f"agreement: every batch of the two feeds equal (images, targets, paths, shapes) {bool(agree)}; images seen {results['pass'][0]} / {results['pass'][1]}; "
                 f"run_batches results equal {results['run_batches'][0] == results['run_batches'][1]}")
    report = "\n".join(lines)
    print(report)
    if args.out:
        Path(args.out).write_text(report + "\n")


if __name__ == "__main__":
    main()
