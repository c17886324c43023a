"""Generate tests/golden/conv_dispatch.json: what the forward / data-gradient conv dispatch of a build of the PARENT commit answers, so that a change of the
dispatch code in csrc/conv.hip, conv_v10.h, conv_strip.h and conv_1x1s.h can be replayed against it (tests/test_host_cpu.py::test_conv_dispatch_table_is_unchanged).

    Y3_LIB=/path/to/the/parent/commit/libyolov3_hip.so python tests/golden/make_conv_dispatch_golden.py

Never from the branch under test: Y3_LIB is required.  No GPU is needed (the queries launch nothing; without a device y3_cu_count() answers 256, an MI355X's count).

Each row is [knob set, dtype, k, s, cin, cout, n, h, w, in_dilation, upsample2x, has_residual, workspace,  variant, rows, tiles, bnin]: the first thirteen are the
question (knob set = index into "knob_sets", dtype = the Y3_* code, workspace 1 = y3_conv_workspace_bytes() bytes; x is (n, h, w, cin) with pitch == cin -- for
in_dilation = 2, the data gradient of a stride-2 layer, (h, w) is the OUTPUT, the forward's input size, and x its stride-2 image), the rest what the library answers:
variant = index into "variants" of y3_conv2d_fwd_variant's name, rows = y3_conv2d_fwd_stats_rows (workspace 0) / _rows_ws (workspace 1), tiles = [n_tiles,
column_blocks, group_blocks] of y3_conv_v10_tiles for a v10 variant (else null), bnin = y3_conv2d_fwd_bnin_rows [without, with] a shortcut for 1x1 stride-1 rows
(else null).
Shapes: every conv of the three model yamls at 640 x 640 and on a map a tenth that size with w != h, at batch 64, 32, 2 and 1, and the same layers as data gradients
(channels swapped; stride-2 layers dilated); both sides of every threshold of the decision; Cin = 8 / 16; a batch beyond the 2 GiB reach of a buffer descriptor; fp32.
Under the default knobs every shape is asked in f16 with the workspace, and without it / with a residual / in bf16 where that changes the answer (and on a few rows
where it does not); under each other knob set the rows whose answer the knob changes, and a few it does not."""
import ctypes as C
import json
import os
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(Path(__file__).resolve().parent))
OUT = Path(__file__).resolve().parent / "conv_dispatch.json"

KNOB_SETS = [{}] + [{k: v} for k, vs in (("conv", (2, 4, 5, 6, 15)), ("conv_strip", (0, 2, 7)), ("conv_v10", (0, 2)), ("v10_half", (0, 1)), ("v10_ksplit", (0, 2)),
                                         ("v10_slices", (1, 3)), ("v10_mp", (6,)), ("v10_blocks", (3,)), ("v10_group", (0,)), ("conv_1x1s", (0, 2))) for v in vs]
VARIANTS = ["direct", "v2", "v2_smallc", "v3_bk64_128x128", "v3_bk32_128x128", "v3_bk32_128x256", "v3_bk32_64x256", "v6", "v10", "v10h", "v10k", "strip", "s1x1"]
F16, BF16, F32 = 0, 1, 2


def questions():
    """(k, s, cin, cout, n, h, w, in_dilation, upsample2x) in the order they are asked"""
    from make_wgrad_dispatch_golden import model_convs

    convs = sorted({c for m in ("yolov3", "yolov3-spp", "yolov3-tiny") for c in model_convs(m)})
    out = []
    for n in (64, 32, 2, 1):
        for k, s, cin, cout, h in convs:
            for hh, ww in ((h, h), (max(2, h // 10), max(2, h // 10) + 3)):
                out.append((k, s, cin, cout, n, hh, ww, 0, 0))
                out.append((k, 1, cout, cin, n, hh, ww, 2 if s == 2 else 0, 0))   # its data gradient
    for cin, cout in ((512, 256), (256, 128)):                                     # the 1x1 layers in front of the two Upsamples
        for n, h in ((64, 20), (2, 20), (64, 40), (1, 40)):
            out.append((1, 1, cin, cout, n, h, h, 0, 1))
    for m in (16384, 16385, 32767, 32768, 65536, 65537):                           # pixel thresholds of the tile choice and of conv_1x1s.h
        for k, cin, cout in ((1, 512, 256), (1, 256, 128), (1, 1024, 512), (3, 512, 384), (3, 64, 128)):
            out.append((k, 1, cin, cout, 1, 1, m, 0, 0))
    for m in (8191, 8192):                                                         # ... of its input-transform form
        out += [(1, 1, 256, 128, 1, 1, m, 0, 0), (1, 1, 128, 64, 1, 1, m, 0, 0)]
    for cin in (128, 256, 512):                                                    # K = 1152, 2304, 4608
        for cout in (128, 384, 512, 640):
            for m in (4096, 65535, 65536):
                out.append((3, 1, cin, cout, 1, 1, m, 0, 0))
    for k, cin in ((1, 64), (3, 64), (1, 256), (3, 32)):                           # 64 / 72 filters
        for cout in (64, 72):
            out += [(k, 1, cin, cout, 2, 40, 52, 0, 0), (k, 1, cin, cout, 64, 160, 160, 0, 0)]
    for cout in (256, 512):                                                        # the quarter round of 256-pixel tiles of conv_v10.h: 64 / cout tiles' worth of pixels
        for cin in (128, 512):
            t = 64 * 256 // cout
            out += [(3, 1, cin, cout, 1, 1, (t - 1) * 256, 0, 0), (3, 1, cin, cout, 1, 1, (t - 1) * 256 + 1, 0, 0), (3, 1, cin, cout, 2, 63, 64, 0, 0), (3, 1, cin, cout, 3, 20, 21, 0, 0)]
    for cin, cout, n, h in ((64, 128, 48, 128), (128, 64, 48, 128), (64, 32, 72, 256), (64, 128, 96, 128)):   # conv_strip.h: T = 24 rows per block x the blocks (one strip per row)
        out += [(3, 1, cin, cout, n, h, 64, 0, 0), (3, 1, cin, cout, n - 1, h, 64, 0, 0), (3, 1, cin, cout, n, h, 65, 0, 0)]
    out += [(3, 2, 64, 128, 48, 256, 128, 0, 0), (3, 2, 64, 128, 47, 256, 128, 0, 0)]
    for cin in (8, 16):                                                            # Cin % 32 != 0: the register-staged kernels, one per filter-count class
        for cout in (16, 32, 64, 128):
            out += [(3, 1, cin, cout, 2, 64, 48, 0, 0), (1, 1, cin, cout, 64, 160, 160, 0, 0), (3, 2, cin, cout, 1, 33, 31, 0, 0)]
    out.append((3, 1, 64, 128, 64, 640, 640, 0, 0))                                # x: 3.4 GB, launched as two image ranges
    out.append((1, 1, 128, 64, 130, 640, 640, 0, 0))                               # x: 13.6 GB, eight ranges with a short last one
    return list(dict.fromkeys(out))


def ask(L, ws_bytes, knobs, dtype, q, res, ws):
    from yolov3_amd import _lib

    k, s, cin, cout, n, h, w, dil, ups = q
    L.y3_tune_reset()
    for key, val in knobs.items():
        assert L.y3_tune_set(key.encode(), val) == 0, key
    if dil == 2:
        x, y = _lib.Y3Tensor(4096, n, (h - 1) // 2 + 1, (w - 1) // 2 + 1, cin, cin), _lib.Y3Tensor(8192, n, h, w, cout, cout)
    else:
        ho, wo = (h + 2 * (k // 2) - k) // s + 1, (w + 2 * (k // 2) - k) // s + 1
        x, y = _lib.Y3Tensor(4096, n, h, w, cin, cin), _lib.Y3Tensor(8192, n, ho * (2 if ups else 1), wo * (2 if ups else 1), cout, cout)
    d = _lib.Y3ConvDesc(dtype, k, s, 0, ups, 0, cin, cout, dil)
    wsb = ws_bytes if ws else 0
    name = C.create_string_buffer(64)
    assert L.y3_conv2d_fwd_variant(C.byref(d), C.byref(x), C.byref(y), res, C.c_size_t(wsb), name, C.c_size_t(64)) == 0, (q, L.y3_last_error())
    variant = VARIANTS.index(name.value.decode())
    rows = L.y3_conv2d_fwd_stats_rows_ws(C.byref(d), C.byref(x), C.byref(y), C.c_size_t(wsb)) if ws else L.y3_conv2d_fwd_stats_rows(C.byref(d), C.byref(x), C.byref(y))
    tiles = None
    if VARIANTS[variant] in ("v10", "v10h", "v10k") and not res:   # (the tile query describes the launch without a residual)
        nt, cb, gb = C.c_int64(0), C.c_int32(0), C.c_int32(0)
        assert L.y3_conv_v10_tiles(C.byref(d), C.byref(x), C.byref(y), C.c_size_t(wsb), None, C.c_int64(0), C.byref(nt), C.byref(cb), C.byref(gb)) == 0, q
        tiles = [nt.value, cb.value, gb.value]
    bnin = None
    if k == 1 and s == 1 and not dil and not ups and dtype != F32:
        yin = _lib.Y3Tensor(12288, n, h, w, cin, cin)
        bnin = [L.y3_conv2d_fwd_bnin_rows(C.byref(d), C.byref(x), C.byref(yin), C.byref(y), sc) for sc in (0, 1)]
    return [variant, rows, tiles, bnin]


def bind(L):
    L.y3_conv_workspace_bytes.restype = C.c_size_t
    L.y3_last_error.restype = C.c_char_p
    L.y3_tune_set.argtypes = [C.c_char_p, C.c_int64]
    L.y3_conv2d_fwd_stats_rows.restype = L.y3_conv2d_fwd_stats_rows_ws.restype = L.y3_conv2d_fwd_bnin_rows.restype = C.c_int64
    return L.y3_conv_workspace_bytes()


def main():
    assert os.environ.get("Y3_LIB"), "point Y3_LIB at the library of the parent commit"
    import torch  # noqa: F401  (its HIP runtime first, as yolov3_amd._lib.lib() loads it)

    L = C.CDLL(os.environ["Y3_LIB"])   # (not _lib.lib(): the parent's library need not export what the branch added)
    ws_bytes = bind(L)
    qs = questions()
    base = {q: ask(L, ws_bytes, {}, F16, q, 0, 1) for q in qs}
    rows = [[0, F16, *q, 0, 1, *base[q]] for q in qs]

    def others(ki, knobs, dtype, res, ws, n_changed, n_same, only=lambda q: True):
        """the rows of a variation of the default question that answer differently, thinned to about n_changed, and about n_same that do not"""
        got = [(q, ask(L, ws_bytes, knobs, dtype, q, res, ws)) for q in qs if only(q)]
        changed = [(q, a) for q, a in got if a != base[q]]
        same = [(q, a) for q, a in got if a == base[q]]
        rows.extend([ki, dtype, *q, res, ws, *a] for q, a in changed[:: max(1, len(changed) // n_changed)] + same[:: max(1, len(same) // n_same)])
        return len(changed)

    others(0, {}, F16, 0, 0, 40, 8)                                   # without the workspace: no K-split form
    others(0, {}, F16, 1, 1, 40, 8, only=lambda q: not q[8])          # with a residual: no strip kernel
    others(0, {}, BF16, 0, 1, 8, 8)
    assert others(0, {}, F32, 0, 1, 12, 1) == len(qs)                 # fp32: the direct kernel, no statistics rows
    changed_by = {ki: others(ki, knobs, F16, 0, 1, 14, 3) for ki, knobs in enumerate(KNOB_SETS[1:], 1)}
    L.y3_tune_reset()
    forms = {v: sum(1 for r in rows if VARIANTS[r[13]] == v) for v in VARIANTS}
    assert all(n >= 5 for n in forms.values()), forms
    assert all(changed_by.values()), changed_by
    assert any(r[14] > 0 and r[6] * r[7] * r[8] * max(r[4], r[5]) * 2 > 2 ** 31 for r in rows), "no statistics rows summed over image ranges"
    head = json.dumps({"columns": "knob_set dtype k s cin cout n h w in_dilation upsample2x has_residual workspace variant rows tiles bnin_rows", "knob_sets": KNOB_SETS,
                       "variants": VARIANTS}, separators=(",", ":"))
    text = head[:-1] + ',"rows":[\n' + ",\n".join(json.dumps(r, separators=(",", ":")) for r in rows) + "]}"
    assert len(text) < 64 * 1024, len(text)
    OUT.write_text(text + "\n")
    print(f"{OUT}: {len(rows)} rows, {len(text)} bytes, rows per variant {forms}, rows a knob set changes {changed_by}")


if __name__ == "__main__":
    main()
