"""CPU tests of the header reader (yolov3_amd/_header.py): the ctypes binding of _lib.py is derived from include/yolov3_hip.h, so these pin the derivation itself --
a handful of signatures written out literally (one per mapping rule), every struct layout against what the host C compiler computes from the same header, and the
refusal of anything the reader does not understand.  No GPU and no library is needed."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from yolov3_amd import _header, _lib

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "yolov3_hip.h"
V, I32, I64, SZ, F = C.c_void_p, C.c_int32, C.c_int64, C.c_size_t, C.c_float
DESC, TENSOR, NMS, LOSS = (C.POINTER(s) for s in (_lib.Y3ConvDesc, _lib.Y3Tensor, _lib.Y3NmsParams, _lib.Y3LossParams))
PINNED = {
    "y3_last_error": (C.c_char_p, []),
    "y3_tune_get": (I64, [C.c_char_p]),
    "y3_conv2d_fwd_ws": (C.c_int, [DESC, TENSOR, V, V, TENSOR, TENSOR, V, SZ, V]),
    "y3_nms": (C.c_int, [V, I32, I32, I32, I32, NMS, V, V, V, V, I64, V, SZ, V]),
    "y3_anchor_metrics": (C.c_int, [V, I64, V, I32, F, V, V, SZ, V]),
    "y3_kmeans_step": (C.c_int, [V, I64, I32, I32, V, V, C.c_uint64, V, V, SZ, V]),
    "y3_loss_fwd": (C.c_int, [LOSS, I32, V, V, I32, V, V, SZ, V]),
    "y3_augment_batch": (C.c_int, [V, I64, V, I64, V, I32, V, I32, I32, V]),
}


def test_pinned_signatures_and_queries():
    assert _lib._H is not None and _lib._SIGNATURES is _lib._H.signatures and _lib.exported_symbols() == list(_lib._SIGNATURES)
    for name, want in PINNED.items():
        assert _lib._SIGNATURES[name] == want, name
    assert _lib._SIGNATURES["y3_tune_reset"] == (None, [])
    # a query is an export without a trailing `void* stream`, read here from the raw text with a regex of the test's own
    text = re.sub(r"/\*.*?\*/", " ", HEADER.read_text(), flags=re.S)
    protos = dict(re.findall(r"\b(y3_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text))
    assert set(protos) == set(_lib._SIGNATURES)
    assert _lib._QUERIES == {n for n, p in protos.items() if not re.search(r"\bvoid\s*\*\s*stream\s*$", p)}
    assert "y3_conv2d_wgrad_last_plan" in _lib._QUERIES and "y3_conv2d_fwd_ws" not in _lib._QUERIES
    assert _lib.ABI_VERSION == 6 and (_lib.Y3_F16, _lib.Y3_BF16, _lib.Y3_F32, _lib.Y3_U8) == (0, 1, 2, 3) and (_lib.Y3_ACT_NONE, _lib.Y3_ACT_SILU) == (0, 1)
    assert (_lib.Y3_ALGO_AUTO, _lib.Y3_ALGO_MFMA, _lib.Y3_ALGO_DIRECT) == (0, 1, 2) and (_lib.Y3_EXPORT_TARGET, _lib.Y3_EXPORT_TXT, _lib.Y3_EXPORT_JSON) == (0, 1, 2)


def _leaves(ctype, prefix="", base=0):
    """(dotted path, offset) of every field of a ctypes Structure, nested structs (first array element) included"""
    for name, t in ctype._fields_:
        off = base + getattr(ctype, name).offset
        yield prefix + name, off
        while issubclass(t, C.Array):
            t = t._type_
        if issubclass(t, C.Structure):
            yield from _leaves(t, prefix + name + ".", off)


def test_layouts_against_the_compiler(tmp_path):
    from yolov3_amd import augment, build, dataset

    structs = _lib._H.structs
    assert [C.sizeof(s) for s in structs.values()] == [32, 48, 40, 32, 40, 280, 1360, 316, 48, 96] and len(structs) == len(re.findall(r"typedef\s+struct", HEADER.read_text()))
    lines = ['#include <stdio.h>', '#include "yolov3_hip.h"', "int main(void) {"]
    for name, s in structs.items():
        lines.append(f'    printf("{name} %zu\\n", sizeof({name}));')
        lines += [f'    printf("{name}.{n} %zu\\n", offsetof({name}, {n}));' for n, _ in s._fields_]
    (tmp_path / "layout.c").write_text("\n".join(lines + ["    return 0;", "}", ""]))
    cc = shutil.which("cc")
    if cc is None:   # ROCm's clang lies beside the hipcc the library is built with
        rocm = Path(build.hipcc()).resolve().parents[1]
        cc = shutil.which("clang", path=os.pathsep.join(str(rocm / d) for d in ("llvm/bin", "lib/llvm/bin")))
    assert cc, "no host C compiler (cc, or ROCm's clang): the layouts cannot be checked"
    subprocess.run([cc, "-std=c11", "-I", str(HEADER.parent), str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")], check=True)
    compiled = {k: int(v) for k, v in (line.split() for line in subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout.splitlines())}
    derived = {}
    for name, s in structs.items():
        derived[name] = C.sizeof(s)
        derived.update({f"{name}.{n}": getattr(s, n).offset for n, _ in s._fields_})
    assert derived == compiled
    # the NumPy records dataset.py / augment.py fill: size and the offset of every field, the nested ones through their parents
    for dt, name in ((augment.TILE, "y3_augment_tile"), (augment.MOSAIC, "y3_augment_mosaic"), (augment.ITEM, "y3_augment_item"), (dataset._RECORD, "y3_dataset_image")):
        assert dt.itemsize == compiled[name] and list(dt.names) == [n for n, _ in structs[name]._fields_]
        for path, off in _leaves(structs[name]):
            sub, at = dt, 0
            for part in path.split("."):
                field = sub.fields[part]
                sub, at = field[0].base, at + field[1]
            assert at == off, (name, path)
            if "." not in path:
                assert at == compiled[f"{name}.{path}"]
    item = np.zeros(2, augment.ITEM)
    assert item["lut"].shape == (2, 3, 256) and item["lut"].dtype == np.uint8 and item["mosaics"]["tiles"]["img"].shape == (2, 2, 4) and item["mosaics"]["inv"].dtype == np.float64
    assert augment.TILE["lpadw"] == np.float32 and dataset._RECORD["offset"] == np.int64 and augment.MOSAIC.fields["tiles"][1] == compiled["y3_augment_mosaic.tiles"]


@pytest.mark.parametrize("snippet, quoted", [
    ("int y3_f(y3_mystery* p, void* stream);", "y3_mystery"),                       # an unknown type
    ("int y3_f(unsigned n, void* stream);", "unsigned"),
    ("int y3_f(void (*done)(int), void* stream);", "(*done)"),                      # a callback parameter
    ("int y3_f(void* stream);\nstatic const int y3_k = 3;", "static const int y3_k = 3"),   # a stray line
    ("int y3_f(void* stream);\n}", "}"),
    ("typedef enum { Y3_A = 0, Y3_B } y3_e;", "Y3_B"),                              # an enumerator without a value
    ("typedef struct { int32_t a; y3_later b; } y3_s;", "y3_later"),
    ("typedef struct { int32_t (*cb)(void); } y3_s;", "(*cb)"),
])
def test_reader_refuses_what_it_does_not_understand(snippet, quoted):
    with pytest.raises(ValueError) as e:
        _header.parse(snippet)
    assert quoted in str(e.value)


def test_reader_on_a_small_header():
    h = _header.parse("""
        #define Y3_ABI_VERSION 9
        #ifdef __cplusplus
        extern "C" {
        #endif
        typedef enum { Y3_X = 2, Y3_Y = -1 } y3_xy;   // both styles of comment are dropped
        enum { Y3_Z = 7 };
        typedef struct { void* data; int32_t n, h, w, c; int32_t pitch; } y3_tensor;
        typedef struct y3_rec { const float* w; uint8_t lut[3][4]; y3_tensor t[2]; double d; } y3_rec;
        /* int y3_not_declared(void); */
        const char* y3_name(void);
        void y3_reset(void);
        size_t y3_bytes(const y3_tensor* t, const y3_rec* device_table, char* out, const void* const* list);
        int y3_go(const y3_tensor* t, float a, double b, uint64_t m,
                  void* stream);
        #ifdef __cplusplus
        }
        #endif
    """)
    assert h.constants == {"Y3_ABI_VERSION": 9, "Y3_X": 2, "Y3_Y": -1, "Y3_Z": 7} and list(h.structs) == ["y3_tensor", "y3_rec"]
    rec, ten = h.structs["y3_rec"], h.structs["y3_tensor"]
    assert [n for n, _ in ten._fields_] == ["data", "n", "h", "w", "c", "pitch"] and C.sizeof(ten) == 32
    assert dict(rec._fields_) == {"w": C.c_void_p, "lut": C.c_uint8 * 4 * 3, "t": ten * 2, "d": C.c_double} and (rec.lut.offset, rec.t.offset, rec.d.offset, C.sizeof(rec)) == (8, 24, 88, 96)
    assert h.signatures == {"y3_name": (C.c_char_p, []), "y3_reset": (None, []), "y3_bytes": (C.c_size_t, [C.POINTER(ten), C.c_void_p, C.c_char_p, C.c_void_p]),
                            "y3_go": (C.c_int, [C.POINTER(ten), C.c_float, C.c_double, C.c_uint64, C.c_void_p])}
    assert h.queries == {"y3_name", "y3_reset", "y3_bytes"}


def test_a_missing_header_names_its_path(tmp_path):
    pkg = tmp_path / "yolov3_amd"
    pkg.mkdir()
    for f in ("_lib.py", "_header.py"):
        shutil.copy(ROOT / "yolov3_amd" / f, pkg / f)
    (pkg / "__init__.py").write_text("")
    code = f"import sys; sys.path.insert(0, {str(tmp_path)!r}); import yolov3_amd._lib"
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert r.returncode != 0 and "Y3Error" in r.stderr and str(tmp_path / "include" / "yolov3_hip.h") in r.stderr
