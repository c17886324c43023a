"""A/B of the filter-bank packers on one MI355X against the PARENT commit's library, never against this tree itself: `--parent` is a clean export of the parent
commit with its library built (python -m yolov3_amd.build there); a child process per arm and round loads either that library (Y3_LIB) or this tree's, the arms
alternating.  A child warms every case up once, then times `--iters` back-to-back calls of each with device events:

    PackJobs.run() and FoldPackJobs.run() on yolov3's full job tables (fp16)
    the five single-layer packers on a 512 -> 1024 3x3 layer (the stem packer on its own 3 -> 32 form), fp16

Pass condition per case: the branch's median over the rounds is no more than the parent's median plus the parent's own max - min.  With --bench the bench.py
figure of both trees is recorded too (each tree's own bench.py and Python).  Nothing here is expected to get faster: the report shows that nothing got slower.

    python tools/filter_bank_ab.py --parent DIR [--rounds 5] [--iters 20] [--bench] [--out profiles/filter_bank_ab.txt]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]


def child(iters: int):
    import torch
    from torch import nn

    sys.path.insert(0, str(ROOT))
    from yolov3_amd import DetectionModel, _lib, engine, ops

    dev, dt = torch.device("cuda:0"), torch.float16
    L, code, st = _lib.lib(), ops.dtype_code(torch.float16), ops.stream_ptr
    torch.manual_seed(0)
    model = DetectionModel("yolov3.yaml", nc=80).to(dev).eval()
    pad8 = lambda n: (n + 7) // 8 * 8   # noqa: E731
    pack = ops.PackJobs(dt, dev)
    for m in model.modules():
        if isinstance(m, nn.Conv2d):
            pack.add(m.weight.detach(), pad8(m.out_channels), pad8(m.in_channels))
    fold = engine.FoldPackJobs(dt, dev)
    layers = [m for m in model.modules() if hasattr(m, "conv") and hasattr(m, "bn")]
    for i, m in enumerate(layers):
        fold.add(m.conv, m.bn, True, stem=i == 0)
    for head in model.model[-1].m:
        fold.add(head, None, False)

    co, ci = 1024, 512
    w = torch.randn(co, ci, 3, 3, device=dev)
    w0 = torch.randn(32, 3, 3, 3, device=dev)
    f = torch.empty(ops.packed_filter_elems(co, ci, 3), dtype=dt, device=dev)
    d = torch.empty(ops.packed_filter_elems(ci, co, 3), dtype=dt, device=dev)
    s2 = torch.empty(int(L.y3_packed_filter_dgrad_s2_elems(co, ci)), dtype=dt, device=dev)
    s0 = torch.empty(int(L.y3_packed_filter_stem_elems(32)), dtype=dt, device=dev)
    cases = {
        "PackJobs.run (yolov3)": pack.run,
        "FoldPackJobs.run (yolov3)": fold.run,
        "y3_pack_filter": lambda: _lib.check(L.y3_pack_filter(w.data_ptr(), co, ci, 3, co, ci, code, f.data_ptr(), st()), "y3_pack_filter"),
        "y3_pack_filter_dgrad": lambda: _lib.check(L.y3_pack_filter_dgrad(w.data_ptr(), co, ci, 3, co, ci, code, d.data_ptr(), st()), "y3_pack_filter_dgrad"),
        "y3_pack_filter_pair": lambda: _lib.check(L.y3_pack_filter_pair(w.data_ptr(), co, ci, 3, co, ci, code, f.data_ptr(), d.data_ptr(), st()), "y3_pack_filter_pair"),
        "y3_pack_filter_dgrad_s2": lambda: _lib.check(L.y3_pack_filter_dgrad_s2(w.data_ptr(), co, ci, co, ci, code, s2.data_ptr(), st()), "y3_pack_filter_dgrad_s2"),
        "y3_pack_filter_stem (3 -> 32)": lambda: _lib.check(L.y3_pack_filter_stem(w0.data_ptr(), 32, 3, 32, code, s0.data_ptr(), st()), "y3_pack_filter_stem"),
    }
    out = {}
    for fn in cases.values():
        fn()
    torch.cuda.synchronize()
    for name, fn in cases.items():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        e1.synchronize()
        out[name] = e0.elapsed_time(e1) / iters
    print("AB " + json.dumps(out), flush=True)


def arm(lib, iters):
    env = dict(os.environ)
    env.pop("Y3_LIB", None)
    if lib is not None:
        env["Y3_LIB"] = str(lib)
    r = subprocess.run([sys.executable, __file__, "--child", "--iters", str(iters)], env=env, capture_output=True, text=True, timeout=300)
    if r.returncode != 0:
        sys.exit(f"the {'parent' if lib else 'branch'} arm failed ({r.returncode}):\n{r.stderr[-2000:]}")
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("AB ")][-1][3:])


def bench(tree):
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "20", "--warmup", "3"], cwd=tree, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        sys.exit(f"bench.py of {tree} failed ({r.returncode}):\n{r.stderr[-2000:]}")
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    return f"{res.get('metric', 'value')} = {res['value']} {res.get('unit', '')}".rstrip()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="clean export of the parent commit, its library built")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--bench", action="store_true", help="also record the bench.py figure of both trees")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "filter_bank_ab.txt"), help="the report is also written to this file ('' for none)")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args.iters)
    parent = Path(args.parent or "").resolve()
    lib = parent / "yolov3_amd" / "lib" / "libyolov3_hip.so"
    assert args.parent and lib.exists(), "--parent: a clean export of the parent commit with its library built"
    assert args.rounds >= 5, "at least five rounds"
    times = ({}, {})   # parent, branch: case -> ms per round
    for r in range(args.rounds):
        for i in ((0, 1) if r % 2 == 0 else (1, 0)):   # the arm that goes first alternates from round to round
            for k, v in arm(lib if i == 0 else None, args.iters).items():
                times[i].setdefault(k, []).append(v)
    lines = [f"filter-bank packers, parent library against this tree: {args.rounds} rounds of one process per arm, arms alternating, {args.iters} calls per case under device events",
             "ms per call: median [min .. max]; pass: branch median <= parent median + (parent max - parent min)",
             f"{'case':32s} {'parent ms':>28s} {'branch ms':>28s} {'branch/parent':>13s} {'bound':>8s}  verdict"]
    bad = []
    for k, tp in times[0].items():
        tb = times[1][k]
        mp, mb, bound = statistics.median(tp), statistics.median(tb), statistics.median(tp) + max(tp) - min(tp)
        ok = mb <= bound
        lines.append(f"{k:32s} {f'{mp:.4f} [{min(tp):.4f} .. {max(tp):.4f}]':>28s} {f'{mb:.4f} [{min(tb):.4f} .. {max(tb):.4f}]':>28s} {mb / mp:13.3f} {bound:8.4f}  {'pass' if ok else 'SLOWER'}")
        if not ok:
            bad.append(k)
    if args.bench:
        lines.append(f"bench.py --gpus 1 --steps 20 --warmup 3: parent {bench(parent)}; branch {bench(ROOT)}")
    lines.append("no case is slower than the parent beyond the parent's own spread" if not bad else "DEFECT: slower than the parent beyond its spread: " + ", ".join(bad))
    report = "\n".join(lines)
    print(report)
    if args.out:
        Path(args.out).write_text(report + "\n")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
