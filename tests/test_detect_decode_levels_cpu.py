"""CPU tests of y3_detect_decode_levels (include/yolov3_hip.h): declared, bound and exported; every refusal happens on the host before anything is launched, so the
argument checks and the eligibility rule of the tiled decode kernel run here without a GPU.  The kernel itself: tests/test_gpu_detect_decode_tile.py."""
import ctypes as C
import re
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]


@pytest.fixture(scope="module")
def lib():
    from yolov3_amd import _lib, build

    build.build(verbose=False)
    return _lib.lib()


def _call(lib, levels, dtype, no=85, na=3, z=1 << 20, raws=None, offs=None, total=1000, n_levels=None):
    """levels: (data pointer, n, h, w, c, pitch) per level.  Pointers are made-up addresses: a call that got as far as a launch would fault, a refusal never touches them."""
    from yolov3_amd import _lib

    nl = len(levels)
    ts = (_lib.Y3Tensor * nl)(*[_lib.Y3Tensor(*lv) for lv in levels])
    anc = (C.c_float * (nl * na * 2))(*([10.0] * (nl * na * 2)))
    st = (C.c_float * nl)(*([8.0] * nl))
    rp = (C.c_void_p * nl)(*(raws or [None] * nl))
    ro = (C.c_int64 * nl)(*(offs or [0] * nl))
    return lib.y3_detect_decode_levels(ts, nl if n_levels is None else n_levels, dtype, na, no, anc, st, rp, z, ro, total, None)


def test_levels_export_is_declared_and_bound(lib):
    from yolov3_amd import _lib, ops

    header = (ROOT / "include" / "yolov3_hip.h").read_text()
    assert re.search(r"\by3_detect_decode_levels\s*\(", header)
    assert "y3_detect_decode_levels" in _lib.exported_symbols() and len(_lib._SIGNATURES["y3_detect_decode_levels"][1]) == 12
    assert lib.y3_abi_version() == 6 == _lib.ABI_VERSION, "an added export: the ABI version stays"
    assert ops.tune_get("decode_tile") == 1
    assert callable(ops.detect_decode_levels)


def test_levels_call_refuses_on_the_host(lib):
    from yolov3_amd import _lib, ops

    F16, F32 = _lib.Y3_F16, _lib.Y3_F32
    ok_level = (1 << 20, 2, 8, 8, 255, 256)
    err = lambda: lib.y3_last_error()
    try:
        assert _call(lib, [ok_level], F32) != 0 and b"2-byte" in err()
        assert _call(lib, [ok_level] * 5, F16, n_levels=6) != 0 and b"levels unsupported" in err()
        assert _call(lib, [ok_level], F16, na=6) != 0 and b"na=6" in err()
        assert _call(lib, [(1 << 20, 2, 8, 8, 200, 256)], F16) != 0 and b"channels" in err()
        assert _call(lib, [ok_level], F16, offs=[900]) != 0 and b"do not fit" in err()
        # the eligibility rule of the tiled kernel: 16-byte aligned head, pitch, raw and z; whole 16-byte groups per (image, anchor) block and in front of the window
        for bad, why in (
            (dict(levels=[(1 << 20, 2, 8, 8, 255, 255)]), b"head is not 16-byte aligned"),
            (dict(levels=[((1 << 20) + 2, 2, 8, 8, 255, 256)]), b"head is not 16-byte aligned"),
            (dict(levels=[ok_level], raws=[(1 << 21) + 8]), b"raw is not 16-byte aligned"),
            (dict(levels=[ok_level], z=(1 << 20) + 2), b"z is not 16-byte aligned"),
            (dict(levels=[ok_level, (1 << 22, 2, 5, 7, 255, 256)], offs=[0, 192]), b"no multiple of 8"),
            (dict(levels=[ok_level], offs=[225]), b"no multiple of 8"),
            (dict(levels=[ok_level], total=999), b"total_rows * no"),
            (dict(levels=[ok_level, (1 << 22, 3, 4, 4, 255, 256)], offs=[0, 192]), b"batch size"),
        ):
            assert _call(lib, dtype=F16, **bad) != 0, bad
            assert b"cannot take the tiled kernel" in err() and why in err(), (bad, err())
        ops.tune_set("decode_tile", 0)
        assert _call(lib, [ok_level], F16) != 0 and b"decode_tile = 0" in err()
    finally:
        ops.tune_reset()
