"""Generate tests/golden/wgrad_dispatch.json: what the filter-gradient dispatch of a build of the PARENT commit answers, so that a change of csrc/train.hip's
dispatch code can be replayed against it (tests/test_host_cpu.py::test_wgrad_dispatch_table_is_unchanged).

    Y3_LIB=/path/to/the/parent/commit/libyolov3_hip.so python tests/golden/make_wgrad_dispatch_golden.py

Never from the branch under test: Y3_LIB is required.  No GPU is needed (the queries launch nothing; without a device y3_cu_count() answers 256, an MI355X's count).

Each row is [knob set, dtype, k, s, cin, cout, n, h, w,  tile, slices, xcd_grouped, workspace_bytes]: the first nine are the question (knob set = index into
"knob_sets", dtype = the Y3_* code, x is (n, h, w, cin) with pitch == cin), the last four what y3_conv2d_wgrad_plan and y3_conv2d_wgrad_workspace_bytes answer.
Shapes: the conv layers of the three model yamls at 640 x 640 and on maps a tenth that size with w != h, at batch 64, 2 and 1; both sides of the thresholds of the
decision (16383 / 16384 pixels, K = 1024 / 1152, 32 / 64 / 128 / 256 filters); one x beyond the 2 GB reach of a buffer descriptor.  Under the default knobs every shape
is kept in f16, bf16 and fp32; under each other knob set the rows whose answer the knob changes, and a few it does not."""
import ctypes as C
import json
import os
import sys
from pathlib import Path

import yaml

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
OUT = Path(__file__).resolve().parent / "wgrad_dispatch.json"

KNOB_SETS = [{}] + [{k: v} for k, vs in (("wgrad", (2, 3, 4)), ("wgrad_patch", (0, 2)), ("wgrad_strip", (0, 2, 7)), ("wgrad_xcd", (0, 1, 3)), ("wgrad_blocks", (1024,))) for v in vs]
KNOB_SETS += [{"wgrad": 3, "wgrad_patch": 0}]   # (the 256-tile kernel shows only where the padded-position kernel does not take the shape first)
F16, BF16, F32 = 0, 1, 2


def pad8(c):
    return -(-c // 8) * 8


def model_convs(name, hw=640):
    """(k, s, cin, cout, h) of every conv of cfg/<name>.yaml at hw x hw, channels padded to 8 as the engines store them"""
    from oracle import yolo_oracle as yo

    layers, _, _, _ = yo.parse_cfg(yaml.safe_load(open(ROOT / "yolov3_amd" / "cfg" / f"{name}.yaml")), 3, 80)
    size, out = {-1: hw}, []
    for L in layers:
        f = L.f if isinstance(L.f, int) else L.f[0]
        h = size[f if f >= 0 else L.i + f] if L.i else hw
        if L.kind == "Conv":
            k, s = L.args[0], (L.args[1] if len(L.args) > 1 else 1)
            out.append((k, s, pad8(L.c1), pad8(L.c2), h))
            h = (h + 2 * (k // 2) - k) // s + 1
        elif L.kind == "Bottleneck":
            out += [(1, 1, L.c1, L.c2 // 2, h), (3, 1, L.c2 // 2, L.c2, h)] * L.n
        elif L.kind == "SPP":
            out += [(1, 1, L.c1, L.c1 // 2, h), (1, 1, L.c1 // 2 * 4, L.c2, h)]
        elif L.kind == "Detect":
            out += [(1, 1, layers[j].c2, 256, size[j]) for j in L.f]
        elif L.kind == "Upsample":
            h *= 2
        elif L.kind == "MaxPool":
            h = (h + 2 * L.args[2] - L.args[0]) // L.args[1] + 1
        elif L.kind == "ZeroPad":
            h += 1
        else:
            assert L.kind == "Concat", L.kind
        size[L.i] = h
    return out


def shapes():
    convs = sorted({c for m in ("yolov3", "yolov3-spp", "yolov3-tiny") for c in model_convs(m)})
    out = []
    for n in (64, 2, 1):
        for k, s, cin, cout, h in convs:
            out.append((k, s, cin, cout, n, h, h))
            out.append((k, s, cin, cout, n, max(2, h // 10), max(2, h // 10) + 3))
    for k, cin in ((1, 1024), (3, 128)):            # K = 1024 / 1152
        for cout in (32, 64, 128, 256):
            for h, w in ((127, 129), (128, 128)):   # 16383 / 16384 pixels
                out.append((k, 1, cin, cout, 1, h, w))
    out.append((1, 1, 4, 4, 1, 8, 16))              # fp32: two slices of the direct kernel whose partials (128 bytes) need less than the 256 bytes of a one-slice launch
    out.append((3, 1, 64, 128, 64, 640, 640))       # x: 3.4 GB
    out.append((3, 1, 32, 64, 64, 640, 640))        # the same map inside the reach
    return list(dict.fromkeys(out))


def main():
    assert os.environ.get("Y3_LIB"), "point Y3_LIB at the library of the parent commit"
    import torch  # noqa: F401  (its HIP runtime first, as yolov3_amd._lib.lib() loads it)

    from yolov3_amd import _lib

    L = C.CDLL(os.environ["Y3_LIB"])   # (not _lib.lib(): the parent's library need not export what the branch added)
    L.y3_conv2d_wgrad_workspace_bytes.restype = C.c_size_t
    L.y3_tune_set.argtypes = [C.c_char_p, C.c_int64]

    def ask(knobs, dtype, shape):
        k, s, cin, cout, n, h, w = shape
        L.y3_tune_reset()
        for key, val in knobs.items():
            assert L.y3_tune_set(key.encode(), val) == 0, key
        d = _lib.Y3ConvDesc(dtype, k, s, 0, 0, 0, cin, cout, 0)
        x = _lib.Y3Tensor(4096, n, h, w, cin, cin)
        tile, slices, xg = C.c_int32(0), C.c_int64(0), C.c_int32(0)
        assert L.y3_conv2d_wgrad_plan(C.byref(d), C.byref(x), C.byref(tile), C.byref(slices), C.byref(xg)) == 0
        return [tile.value, slices.value, xg.value, L.y3_conv2d_wgrad_workspace_bytes(C.byref(d), C.byref(x))]

    all_shapes = shapes()
    base = {sh: ask({}, F16, sh) for sh in all_shapes}
    rows = [[0, F16, *sh, *base[sh]] for sh in all_shapes]
    for dtype in (BF16, F32):
        rows += [[0, dtype, *sh, *ask({}, dtype, sh)] for sh in all_shapes]
    changed_by = {}
    for ki, knobs in enumerate(KNOB_SETS[1:], 1):
        got = [(sh, ask(knobs, F16, sh)) for sh in all_shapes]
        changed = [(sh, a) for sh, a in got if a != base[sh]]
        same = [(sh, a) for sh, a in got if a == base[sh]]
        changed_by[ki] = len(changed)
        rows += [[ki, F16, *sh, *a] for sh, a in changed[:: max(1, len(changed) // 24)] + same[:: max(1, len(same) // 4)]]
    L.y3_tune_reset()
    forms = {t: sum(1 for r in rows if r[9] == t) for t in (0, 3, 4, 128, 256)}
    assert all(v >= 10 for v in forms.values()), forms
    for key in {k for ks in KNOB_SETS for k in ks}:
        assert any(changed_by[ki] for ki, ks in enumerate(KNOB_SETS) if ki and key in ks), f"knob {key} changes no answer"
    assert all(changed_by[ki] for ki in changed_by), changed_by
    text = json.dumps({"columns": "knob_set dtype k s cin cout n h w tile slices xcd_grouped workspace_bytes", "knob_sets": KNOB_SETS, "rows": rows}, separators=(",", ":"))
    text = text.replace("],[", "],\n[")
    assert len(text) < 64 * 1024, len(text)
    OUT.write_text(text + "\n")
    print(f"{OUT}: {len(rows)} rows, {len(text)} bytes, rows per form {forms}, rows a knob set changes {changed_by}")


if __name__ == "__main__":
    main()
