"""A/B of copy-paste in one train-mode batch on one MI355X, in interleaved rounds (csrc/augment.hip through yolov3_amd/augment.py).  Synthetic set as
tools/augment_polygons_ab.py makes it: --images seeded images whose long side is --imgsz, about --labels-per-image labels each, every label a polygon of 20 to 200
vertices; batches of --batch, the augmentation values of data/hyps/hyp.scratch-low.yaml plus copy_paste.

  (a) parent   with --parent-lib (a libyolov3_hip.so built from the parent commit): the launches of a batch WITHOUT pastes -- y3_augment_batch and y3_augment_targets of
               the box-only set, y3_augment_polygons and y3_augment_targets_polygons of the polygon set -- through this commit's library and through the parent's, loaded
               side by side and alternated (the order of the arms reversed every other round).  The guard: this commit's median lies within the min .. max of the
               parent arm's own rounds.  The comparison is repeated --guard-runs times in the same process and EVERY repetition is reported, with the difference of
               the medians per repetition: the two builds' instruction lists differ slightly ("Copy-paste, measured"), so the guard is decided on all of them, not on one.
  (b) pastes   the polygon set at copy_paste 0.1 and 0.5: the five launches of the copy-paste form one by one (the clearing of the masks with the raster), against
               the three launches the SAME records take without their candidates; the extra time per batch and, with --step-ms, its share of the train step
  (c) host     the same batch through the NumPy statement of tests/augment_copy_paste_cases.py, one process, once per setting, for scale

Images, targets, accepted lists and masks of the device must equal the statement's bit for bit before anything is timed.  No number is promised: the report records
what was measured.

    timeout -k 10 900 python tools/augment_copy_paste_ab.py [--images 512] [--imgsz 640] [--batch 64] [--rounds 6] [--guard-runs 5] [--step-ms 55] [--parent-lib PATH] [--out profiles/augment_copy_paste_ab.txt]
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
sys.path.insert(0, str(ROOT / "tools"))

import augment_cases as ac  # noqa: E402
import augment_copy_paste_cases as cpc  # noqa: E402
from augment_polygons_ab import synthetic_set  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=512)
    ap.add_argument("--imgsz", type=int, default=640)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--labels-per-image", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--launches", type=int, default=20, help="launches timed per round and arm")
    ap.add_argument("--guard-runs", type=int, default=5, help="repetitions of the comparison with the parent's library, each of --rounds rounds; all are reported")
    ap.add_argument("--step-ms", type=float, default=0.0, help="the train step of the same batch size on the same machine (bench.py --mode train), for the share")
    ap.add_argument("--parent-lib", default="", help="libyolov3_hip.so of the parent commit: the launches of a batch without pastes are compared with it")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "augment_copy_paste_ab.txt"), help="the report is also written to this file ('' for none)")
    args = ap.parse_args()
    assert args.rounds >= 5, "at least five rounds per arm"

    from yolov3_amd import DeviceTrainDataset, _lib, augment, ops   # noqa: E402

    assert torch.cuda.is_available(), "augment_copy_paste_ab.py measures on an MI355X; there is nothing to measure without one"
    dev = torch.device("cuda:0")
    n, S, bs = args.images, args.imgsz, args.batch
    images, labels, segments, hw = synthetic_set(n, S, args.labels_per_image, np.random.RandomState(0))
    low = dict(ac.CASES["low"]["hyp"])
    lib, med, st_ptr = _lib.lib(), statistics.median, ops.stream_ptr

    def events(fn, count):
        """milliseconds per call of `count` calls of fn, by device events"""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(count):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / count

    def rounds(arms):
        for fn in arms.values():   # untimed
            assert fn() in (0, None)
        times = {k: [] for k in arms}
        for r in range(args.rounds):
            for name, fn in (list(arms.items())[::-1] if r % 2 else arms.items()):   # the arms in turn, the order reversed every other round
                times[name].append(events(fn, args.launches))
        return times

    lines = [f"augment copy-paste A/B: {n} cached images (long side {S}), {sum(len(l) for l in labels)} labels, every label a polygon of 20 .. 200 vertices, batches of {bs}, "
             f"hyp low, {args.rounds} interleaved rounds of {args.launches} launches per arm, {torch.cuda.get_device_name(0)}"]

    # ---- (a) a batch without pastes against the parent's library -----------------------------------------------------------------------------------------------------
    ds0 = DeviceTrainDataset(images, labels, low, img_size=S, batch_size=bs, device=dev, segments=segments, copy_paste=True)   # copy_paste 0 in the hyp: today's launches
    box = DeviceTrainDataset(images, labels, low, img_size=S, batch_size=bs, device=dev)
    random.seed(0)
    np.random.seed(0)
    items = ds0.draw_batch(0)
    upper = int(sum(len(labels[j]) for it in items for mo in it.mosaics for j in mo.indices))
    rec = torch.from_numpy(augment.pack_items(items).view(np.uint8).copy()).to(dev)
    out = torch.empty((len(items), 3, S, S), dtype=torch.uint8, device=dev)
    tg, of = torch.empty(upper, 6, dtype=torch.float32, device=dev), torch.empty(len(items) + 1, dtype=torch.int64, device=dev)
    bx, ins, pw = torch.empty(upper, 4, dtype=torch.float64, device=dev), torch.empty(upper, dtype=torch.int32, device=dev), torch.empty(len(items), 2, dtype=torch.int32, device=dev)

    def plain_arms(L, d, prefix=""):
        """the four launches of a batch without pastes through library L, into buffers allocated once"""
        verts = (d._vertices.data_ptr(), d._vertices.shape[0], d._vertex_offsets.data_ptr(), d._vertex_offsets.numel() - 1)
        return {
            prefix + "y3_augment_batch": lambda: L.y3_augment_batch(box._arena.data_ptr(), box._arena.numel(), box._records.data_ptr(), box.n, rec.data_ptr(), len(items), out.data_ptr(), 3, S, st_ptr()),
            prefix + "y3_augment_targets": lambda: L.y3_augment_targets(box._labels.data_ptr(), box._label_offsets.data_ptr(), box._records.data_ptr(), box.n, rec.data_ptr(), len(items), S,
                                                                        tg.data_ptr(), upper, of.data_ptr(), st_ptr()),
            prefix + "y3_augment_polygons": lambda: L.y3_augment_polygons(*verts, d._label_offsets.data_ptr(), d._records.data_ptr(), d.n, rec.data_ptr(), len(items), S, bx.data_ptr(),
                                                                          ins.data_ptr(), pw.data_ptr(), upper, st_ptr()),
            prefix + "y3_augment_targets_polygons": lambda: L.y3_augment_targets_polygons(d._labels.data_ptr(), d._label_offsets.data_ptr(), d._records.data_ptr(), d.n, rec.data_ptr(), len(items),
                                                                                          S, bx.data_ptr(), ins.data_ptr(), pw.data_ptr(), tg.data_ptr(), upper, of.data_ptr(), st_ptr()),
        }

    arms = plain_arms(lib, ds0)
    if args.parent_lib:
        parent = ctypes.CDLL(args.parent_lib)
        for name in arms:
            getattr(parent, name).restype, getattr(parent, name).argtypes = _lib._SIGNATURES[name]
        mine = {}
        for name, fn in arms.items():   # equal bytes first
            assert fn() == 0
            mine[name] = [t.clone() for t in (out, tg, of, bx, ins, pw)]
        for name, fn in plain_arms(parent, ds0).items():
            for t in {"y3_augment_batch": (out,), "y3_augment_polygons": (bx, ins, pw)}.get(name, (tg,)):   # what this launch writes (the polygon targets read the workspace before them)
                t.zero_()
            assert fn() == 0
            nl = int(of.cpu()[-1]) if "targets" in name else 0
            same = {"y3_augment_batch": lambda m: torch.equal(m[0], out), "y3_augment_polygons": lambda m: torch.equal(m[5], pw) and torch.equal(m[4], ins) and torch.equal(m[3].view(torch.int64), bx.view(torch.int64))}
            ok = same[name](mine[name]) if name in same else torch.equal(mine[name][2], of) and torch.equal(mine[name][1][:nl].view(torch.int32), tg[:nl].view(torch.int32))
            assert ok, f"{name}: this commit's output differs from the parent's"
        lines.append("(a) a batch without pastes, this commit against the PARENT commit's library (outputs equal byte for byte first):")
        arms.update(plain_arms(parent, ds0, "parent "))
    inside, diffs = {k: 0 for k in list(arms)[:4]}, {k: [] for k in list(arms)[:4]}
    for run in range(args.guard_runs if args.parent_lib else 1):
        times = rounds(arms)
        lines.append(f"  repetition {run + 1} of {args.guard_runs if args.parent_lib else 1}:")
        for name, v in times.items():
            lines.append(f"    {name:40s} {med(v) * 1e3:9.1f} us   (rounds {min(v) * 1e3:.1f} .. {max(v) * 1e3:.1f})")
        if args.parent_lib:
            for name in inside:
                a, b = times[name], times["parent " + name]
                ok = min(b) <= med(a) <= max(b)
                inside[name] += ok
                diffs[name].append((med(a) - med(b)) * 1e3)
                lines.append(f"    guard {name}: median {med(a) * 1e3:.1f} us within the parent's rounds {min(b) * 1e3:.1f} .. {max(b) * 1e3:.1f} us: {ok} "
                             f"(difference of the medians {diffs[name][-1]:+.1f} us)")
    if args.parent_lib:
        for name, k in inside.items():
            d = diffs[name]
            lines.append(f"  guard {name}: inside in {k} of {args.guard_runs} repetitions; differences of the medians {', '.join(f'{v:+.1f}' for v in d)} us "
                         f"(median {med(d):+.1f}, {sum(v > 0 for v in d)} positive, {sum(v < 0 for v in d)} negative)")

    # ---- (b), (c) the polygon set at copy_paste 0.1 and 0.5 -------------------------------------------------------------------------------------------------------------
    for p in (0.1, 0.5):
        ds = DeviceTrainDataset(images, labels, dict(low, copy_paste=p), img_size=S, batch_size=bs, device=dev, segments=segments, copy_paste=True)
        random.seed(0)
        np.random.seed(0)
        items = ds.draw_batch(0)
        table, nk, n_masks = augment.pack_paste(items)
        upper = int(sum(len(labels[j]) for it in items for mo in it.mosaics for j in mo.indices))
        im, targets, _, _ = ds.get_batch(0, items=items)
        sel_i, sel_f, masks = (t.clone() for t in ds.pastes)
        t0 = time.perf_counter()
        st = cpc.batch_statement(items, images, labels, segments, hw, S)
        t_host = time.perf_counter() - t0
        bits = ((masks.cpu().unsqueeze(-1) >> torch.arange(32, dtype=torch.int32)) & 1).bool().reshape(n_masks, 2 * S, 2 * S).numpy()
        acc = [[(e, int(sel_i[int(table[s]) + e, 1])) for e in range(int(table[s + 1] - table[s])) if int(sel_i[int(table[s]) + e, 0])] for s in range(2 * len(items))]
        agree = (np.array_equal(im.cpu().numpy(), st["im"]) and np.array_equal(targets.cpu().numpy().view(np.int32), st["targets"].view(np.int32))
                 and acc == [[(e, j) for e, j, _ in a] for a in st["accepted"]]
                 and all(np.array_equal(bits[int(table[2 * len(items) + 1 + s])], m) for s, m in enumerate(st["masks"]) if m is not None))
        assert agree, f"copy_paste {p}: the device and the statement differ: nothing is timed"
        rec = torch.from_numpy(augment.pack_items(items).view(np.uint8).copy()).to(dev)
        paste = torch.from_numpy(table).to(dev)
        rows = upper + nk
        tg, of = torch.empty(rows, 6, dtype=torch.float32, device=dev), torch.empty(len(items) + 1, dtype=torch.int64, device=dev)
        bx, ins, pw = torch.empty(rows, 4, dtype=torch.float64, device=dev), torch.empty(rows, dtype=torch.int32, device=dev), torch.empty(len(items), 2, dtype=torch.int32, device=dev)
        verts = (ds._vertices.data_ptr(), ds._vertices.shape[0], ds._vertex_offsets.data_ptr(), ds._vertex_offsets.numel() - 1)
        batch = (ds._records.data_ptr(), ds.n, rec.data_ptr(), len(items), S, paste.data_ptr(), nk)

        def raster():
            masks.zero_()
            return lib.y3_augment_copy_paste_raster(*verts, ds._label_offsets.data_ptr(), *batch, sel_i.data_ptr(), masks.data_ptr(), n_masks, st_ptr())

        arms = {
            "y3_augment_copy_paste_select": lambda: lib.y3_augment_copy_paste_select(ds._labels.data_ptr(), ds._label_offsets.data_ptr(), verts[2], verts[1], verts[3], *batch, sel_i.data_ptr(),
                                                                                     sel_f.data_ptr(), st_ptr()),
            "masks.zero_ + y3_augment_copy_paste_raster": raster,
            "y3_augment_batch_paste": lambda: lib.y3_augment_batch_paste(ds._arena.data_ptr(), ds._arena.numel(), ds._records.data_ptr(), ds.n, rec.data_ptr(), len(items), out.data_ptr(), 3, S,
                                                                         paste.data_ptr(), masks.data_ptr(), n_masks, st_ptr()),
            "y3_augment_polygons_paste": lambda: lib.y3_augment_polygons_paste(*verts, ds._label_offsets.data_ptr(), *batch, sel_i.data_ptr(), sel_f.data_ptr(), bx.data_ptr(), ins.data_ptr(),
                                                                               pw.data_ptr(), rows, st_ptr()),
            "y3_augment_targets_paste": lambda: lib.y3_augment_targets_paste(ds._labels.data_ptr(), ds._label_offsets.data_ptr(), *batch, sel_i.data_ptr(), sel_f.data_ptr(), bx.data_ptr(),
                                                                             ins.data_ptr(), pw.data_ptr(), tg.data_ptr(), rows, of.data_ptr(), st_ptr()),
            "same records, no candidates: y3_augment_batch": lambda: lib.y3_augment_batch(ds._arena.data_ptr(), ds._arena.numel(), ds._records.data_ptr(), ds.n, rec.data_ptr(), len(items),
                                                                                          out.data_ptr(), 3, S, st_ptr()),
            "same records, no candidates: y3_augment_polygons": lambda: lib.y3_augment_polygons(*verts, ds._label_offsets.data_ptr(), ds._records.data_ptr(), ds.n, rec.data_ptr(), len(items), S,
                                                                                                bx.data_ptr(), ins.data_ptr(), pw.data_ptr(), upper, st_ptr()),
            "same records, no candidates: y3_augment_targets_polygons": lambda: lib.y3_augment_targets_polygons(ds._labels.data_ptr(), ds._label_offsets.data_ptr(), ds._records.data_ptr(), ds.n,
                                                                                                                rec.data_ptr(), len(items), S, bx.data_ptr(), ins.data_ptr(), pw.data_ptr(),
                                                                                                                tg.data_ptr(), upper, of.data_ptr(), st_ptr()),
        }
        times = rounds(arms)
        accepted = int(sel_i[:, 0].sum())
        lines.append(f"(b) copy_paste {p}: {nk} candidates in {n_masks} of {sum(len(it.mosaics) for it in items)} mosaics, {accepted} accepted, {upper} label rows in the tiles, "
                     f"{len(targets)} survivors, masks {masks.numel() * 4 / 1e6:.1f} MB; images, targets, accepted lists and masks equal the statement bit for bit {bool(agree)}")
        for name, v in times.items():
            lines.append(f"  {name:58s} {med(v) * 1e3:9.1f} us   (rounds {min(v) * 1e3:.1f} .. {max(v) * 1e3:.1f})")
        names = list(arms)
        extra = sum(med(times[k]) for k in names[:5]) - sum(med(times[k]) for k in names[5:])
        lines.append(f"  extra per batch at copy_paste {p} (the five launches - the three without candidates): {extra * 1e3:.1f} us"
                     + (f", {extra / args.step_ms * 100:.2f} % of a {args.step_ms:.1f} ms train step of batch {bs}" if args.step_ms else ""))
        lines.append(f"(c) copy_paste {p}: the same batch through the NumPy statement on the host (images, labels, rasters; one process, one run): {t_host:.1f} s")
    report = "\n".join(lines)
    print(report)
    if args.out:
        Path(args.out).write_text(report + "\n")


if __name__ == "__main__":
    main()
