"""CPU side of the head-first NMS (knob nms_head): the knob is registered, and the workspace a caller has to give never
shrank -- the control words of the two rounds were added to it, and a caller that sized its buffer once keeps working."""
import ctypes as C

import pytest

# (bs, n_rows, nc, multi_label, capacity) -> y3_nms_workspace_bytes before the control block of the two rounds was added
BEFORE = [
    ((1, 1, 1, 0, 0), 80128),
    ((1, 10, 80, 1, 0), 80128),
    ((2, 2535, 80, 1, 0), 2564864),
    ((3, 4000, 3, 1, 0), 2870016),
    ((4, 4000, 20, 1, 70000), 5520640),
    ((32, 25200, 80, 1, 0), 46830336),
    ((32, 25200, 80, 1, 500000), 44961024),
    ((5, 3000, 10, 1, 0), 6429696),
    ((64, 25200, 80, 0, 0), 93659904),
    ((2, 1500, 600, 1, 0), 2547968),
]


@pytest.fixture(scope="module")
def lib():
    from yolov3_amd import _lib, build

    build.build(verbose=False)
    return _lib.lib()


def test_nms_head_knob_is_registered(lib):
    from yolov3_amd import ops

    try:
        default = ops.tune_get("nms_head")
        assert default > 0 and default % 64 == 0, default   # a head in whole groups of 64 ranks
        ops.tune_set("nms_head", 0)
        assert ops.tune_get("nms_head") == 0
        ops.tune_set("nms_head", -128)
        assert ops.tune_get("nms_head") == -128
    finally:
        ops.tune_reset()
    assert ops.tune_get("nms_head") == default


@pytest.mark.parametrize("args,before", BEFORE, ids=[str(a) for a, _ in BEFORE])
def test_nms_workspace_did_not_shrink(lib, args, before):
    from yolov3_amd import _lib

    bs, n_rows, nc, multi, cap = args
    p = _lib.Y3NmsParams(0.6, 0.001, multi, 0, 300, 30000, 7680.0, 0)
    now = int(lib.y3_nms_workspace_bytes(bs, n_rows, nc, C.byref(p), cap))
    assert now >= before, (now, before)
    assert now - before <= 4 * (130 * bs + 1) + 512, (now, before)   # ... and grew by the control words (130 per image) and alignment only
