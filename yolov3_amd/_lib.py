"""ctypes binding of libyolov3_hip.so (include/yolov3_hip.h).  There is NO fallback: if the library is
missing or a symbol is absent this module raises -- the product path never routes around the HIP code."""
from __future__ import annotations

import ctypes as C
import os
import threading
from pathlib import Path

from . import _header

_PKG = Path(__file__).resolve().parent
LIB_PATH = Path(os.environ["Y3_LIB"]) if os.environ.get("Y3_LIB") else _PKG / "lib" / "libyolov3_hip.so"  # Y3_LIB: instrumented debug builds (tools/timeline.py)
HEADER_PATH = _PKG.parent / "include" / "yolov3_hip.h"


class Y3Error(RuntimeError):
    pass


# Constants, structs, signatures and queries are all read, once per process, from the one file the C side is compiled against.
if not HEADER_PATH.exists():
    raise Y3Error(f"{HEADER_PATH} is missing: the bindings are read from the header the library is compiled against")
_H = _header.parse(HEADER_PATH.read_text())
_K = _H.constants
ABI_VERSION = _K["Y3_ABI_VERSION"]
Y3_F16, Y3_BF16, Y3_F32, Y3_U8 = _K["Y3_F16"], _K["Y3_BF16"], _K["Y3_F32"], _K["Y3_U8"]
Y3_ACT_NONE, Y3_ACT_SILU = _K["Y3_ACT_NONE"], _K["Y3_ACT_SILU"]
Y3_ALGO_AUTO, Y3_ALGO_MFMA, Y3_ALGO_DIRECT = _K["Y3_ALGO_AUTO"], _K["Y3_ALGO_MFMA"], _K["Y3_ALGO_DIRECT"]
Y3_EXPORT_TARGET, Y3_EXPORT_TXT, Y3_EXPORT_JSON = _K["Y3_EXPORT_TARGET"], _K["Y3_EXPORT_TXT"], _K["Y3_EXPORT_JSON"]   # y3_export_rows `form`
Y3Tensor = _H.structs["y3_tensor"]
Y3ConvDesc = _H.structs["y3_conv_desc"]
Y3NmsParams = _H.structs["y3_nms_params"]
Y3LossParams = _H.structs["y3_loss_params"]
Y3PackJob = _H.structs["y3_pack_job"]             # one record of the device table of y3_pack_filter_jobs
Y3FoldPackJob = _H.structs["y3_fold_pack_job"]    # one record of the device table of y3_fold_pack_jobs
Y3DatasetImage = _H.structs["y3_dataset_image"]   # the device records of dataset.py / augment.py, filled through np.dtype(...)
Y3AugmentTile = _H.structs["y3_augment_tile"]
Y3AugmentMosaic = _H.structs["y3_augment_mosaic"]
Y3AugmentItem = _H.structs["y3_augment_item"]
_SIGNATURES = _H.signatures   # symbol -> (restype, argtypes): every export the header declares, all REQUIRED
_QUERIES = _H.queries         # exports without a trailing `void* stream` launch nothing (sizes, plans, names, knobs): CallTimer does not time them

_lib = None


def exported_symbols():
    return list(_SIGNATURES)


def lib() -> C.CDLL:
    """Load libyolov3_hip.so (once).  Import torch first so the HIP runtime torch ships is the one the library
    binds to (same SONAME libamdhip64.so.7): streams and device pointers then belong to one runtime."""
    global _lib
    if _lib is not None:
        t = _call_timer
        return _lib if t is None else t
    import torch  # noqa: F401  (must precede the dlopen, see docstring)

    if not LIB_PATH.exists():
        raise Y3Error(
            f"{LIB_PATH} is missing: the MI355X HIP library has not been built. Run `python -m yolov3_amd.build` "
            "(needs hipcc, gfx950). There is no CPU or PyTorch fallback for this path."
        )
    handle = C.CDLL(str(LIB_PATH))
    for name, (res, args) in _SIGNATURES.items():
        try:
            fn = getattr(handle, name)
        except AttributeError as e:
            raise Y3Error(f"{LIB_PATH} does not export {name}; rebuild with `python -m yolov3_amd.build --force`") from e
        fn.restype, fn.argtypes = res, args
    if handle.y3_abi_version() != ABI_VERSION:
        raise Y3Error(f"ABI version mismatch: library reports {handle.y3_abi_version()}, bindings expect {ABI_VERSION}")
    _lib = handle
    return handle


_call_timer = None


class CallTimer:
    """HIP-event timing of every C-ABI call made while the timer is installed (`with CallTimer() as t: step()`), on the stream the kernels are launched on (torch's
    current stream: what ops.stream_ptr() hands to the library).  bench.py uses it to split ONE training step into kernel families in the run that reports it,
    instead of quoting a profile taken elsewhere.  `by_function()` -> {C function: [milliseconds, calls]} once the stream has drained.  Bench-only: while it
    is installed EVERY thread's calls are timed (autograd runs the backward on its own thread), each on the stream current in that thread; code that cached the real handle
    before bypasses it; it stops recording at MAX_RECORDS."""

    MAX_RECORDS = 100_000   # bench-only tool: a timer left installed around a long loop stops recording instead of growing without bound

    def __init__(self):
        self.records = []   # (function name, start event, end event)
        self._fns = {}
        self._lock = threading.Lock()         # the backward of a step runs on autograd's own thread: every thread of the process is timed, appends are serialised
        self.dropped = 0

    def __getattr__(self, name):   # stands in for the ctypes handle: lib().y3_xxx(...)
        fn = self._fns.get(name)
        if fn is None:
            import torch

            raw = getattr(_lib, name)
            if name in _QUERIES:
                fn = raw          # queries: nothing is launched
            else:
                def fn(*a, raw_=raw, name_=name):
                    if len(self.records) >= self.MAX_RECORDS:
                        self.dropped += 1
                        return raw_(*a)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    r = raw_(*a)
                    e1.record()
                    with self._lock:
                        self.records.append((name_, e0, e1))
                    return r
            self._fns[name] = fn
        return fn

    def __enter__(self):
        global _call_timer
        lib()   # (loaded before the proxy stands in for it)
        _call_timer = self
        return self

    def __exit__(self, *exc):
        global _call_timer
        _call_timer = None
        return False

    def by_function(self):
        import torch

        torch.cuda.synchronize()
        out = {}
        for name, e0, e1 in self.records:
            a = out.setdefault(name, [0.0, 0])
            a[0] += e0.elapsed_time(e1)
            a[1] += 1
        return out


def check(status: int, what: str = ""):
    if status != 0:
        msg = lib().y3_last_error().decode(errors="replace")
        raise Y3Error(f"{what}: {msg}" if what else msg)
