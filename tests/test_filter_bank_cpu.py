"""CPU tests of the filter-bank surface (csrc/filter_bank.h, csrc/filter_bank.hip): the size queries against the torch restatement of tests/filter_bank_cases.py,
and the ctypes job records of ops.PackJobs / engine.FoldPackJobs against the byte layout of the C structs (the struct formats both tables were written with before)."""
import ctypes
import struct
import sys
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests"))

import filter_bank_cases as fb  # noqa: E402


@pytest.fixture(scope="module")
def lib():
    from yolov3_amd import _lib, build

    build.build(verbose=False)
    return _lib.lib()


def test_filter_bank_is_a_translation_unit_without_extra_flags():
    assert ("filter_bank.hip", []) in __import__("yolov3_amd.build", fromlist=["SOURCES"]).SOURCES


@pytest.mark.parametrize("case", fb.GENERIC, ids=str)
def test_generic_bank_sizes(lib, case):
    co, ci, k, cout, cin = case
    w = fb.weights((co, ci, k, k))
    assert fb.ref_fwd(w, cout, cin, torch.float16).numel() == lib.y3_packed_filter_elems(cout, cin, k)
    assert fb.ref_dgrad(w, cout, cin, torch.float16).numel() == lib.y3_packed_filter_elems(cin, cout, k)


@pytest.mark.parametrize("case", fb.STEM, ids=str)
def test_stem_bank_sizes(lib, case):
    co, ci, cout = case
    assert fb.ref_stem(fb.weights((co, ci, 3, 3)), cout, torch.float16).numel() == lib.y3_packed_filter_stem_elems(cout)


@pytest.mark.parametrize("case", fb.STRIDE2, ids=str)
def test_stride2_bank_sizes(lib, case):
    co, ci, cout, cin = case
    assert fb.ref_dgrad_s2(fb.weights((co, ci, 3, 3)), cout, cin, torch.float16).numel() == lib.y3_packed_filter_dgrad_s2_elems(cout, cin)


def test_job_records_have_the_bytes_of_the_c_structs():
    from yolov3_amd import _lib

    assert ctypes.sizeof(_lib.Y3PackJob) == 48 and ctypes.sizeof(_lib.Y3FoldPackJob) == 96
    p = [0x7F0012345600 + 256 * i for i in range(8)]
    job = (p[0], p[1], 0, 21, 8, 3, 24, 8, 1234)
    assert bytes(_lib.Y3PackJob(*job)) == struct.pack("<QQQ6i", *job)
    fold = (p[0], 0, p[2], p[3], p[4], p[5], p[6], p[7], 1e-3, 255, 64, 1, 256, 64, 0, 77)
    assert bytes(_lib.Y3FoldPackJob(*fold)) == struct.pack("<8Qf7i", *fold)
    stem = (p[0], p[1], 0, 0, 0, 0, p[6], p[7], 0.0, 32, 3, 3, 32, 8, 1, 0)
    assert bytes(_lib.Y3FoldPackJob(*stem)) == struct.pack("<8Qf7i", *stem)
