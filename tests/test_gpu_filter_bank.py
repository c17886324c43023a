"""Every filter-bank packer on the MI355X against the torch restatement of the layouts (tests/filter_bank_cases.py), bit for bit: the five single-layer packers
(into banks pre-filled with a sentinel: they write the whole bank, padding = 0) and the two job launches (into the zero-filled banks their Python owners allocate).
The one exception to "the whole bank": the tail of a fragment-ordered copy behind a K-padded bank (fb.frag_tail), which nothing writes and nothing reads."""
import sys
from pathlib import Path

import pytest
import torch
from torch import nn

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests"))

import filter_bank_cases as fb  # noqa: E402

HALVES = [torch.float16, torch.bfloat16]
SENTINEL = 7.0
_REF: dict = {}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


def ref(kind, case, dtype):
    """the expected bank of a case, computed once and never modified"""
    key = (kind, case, dtype)
    if key not in _REF:
        if kind == "stem":
            _REF[key] = fb.ref_stem(fb.weights(case[:2] + (3, 3)), case[2], dtype)
        elif kind == "s2":
            _REF[key] = fb.ref_dgrad_s2(fb.weights(case[:2] + (3, 3)), case[2], case[3], dtype)
        else:
            co, ci, k, cout, cin = case
            _REF[key] = (fb.ref_fwd if kind == "fwd" else fb.ref_dgrad)(fb.weights((co, ci, k, k)), cout, cin, dtype)
    return _REF[key]


def assert_bits(got, want, what, tail=0):
    ints = torch.int32 if want.dtype == torch.float32 else torch.int16
    assert got.dtype == want.dtype and got.numel() == want.numel(), what
    n = want.numel() - tail
    g, w = got.cpu().view(ints)[:n], want.view(ints)[:n]
    assert torch.equal(g, w), f"{what}: {int((g != w).sum())} of {n} elements differ"


def sentinel_bank(n, dtype, dev):
    return torch.full((int(n),), SENTINEL, dtype=dtype, device=dev)


@pytest.mark.parametrize("dtype", HALVES + [torch.float32], ids=["fp16", "bf16", "fp32"])
def test_forward_and_data_gradient_banks(dev, dtype):
    from yolov3_amd import _lib, ops

    L, code = _lib.lib(), ops.dtype_code(dtype)
    for case in fb.GENERIC:
        co, ci, k, cout, cin = case
        w = fb.weights((co, ci, k, k)).to(dev)
        tf, td = fb.frag_tail(cout, cin, k), fb.frag_tail(cin, cout, k)
        assert_bits(ops.pack_filter(w, cout, cin, dtype), ref("fwd", case, dtype), f"pack_filter {case}", tf)
        assert_bits(ops.pack_filter_dgrad(w, cout, cin, dtype), ref("dgrad", case, dtype), f"pack_filter_dgrad {case}", td)
        f, d = sentinel_bank(ops.packed_filter_elems(cout, cin, k), dtype, dev), sentinel_bank(ops.packed_filter_elems(cin, cout, k), dtype, dev)
        _lib.check(L.y3_pack_filter(w.data_ptr(), co, ci, k, cout, cin, code, f.data_ptr(), ops.stream_ptr()), "y3_pack_filter")
        _lib.check(L.y3_pack_filter_dgrad(w.data_ptr(), co, ci, k, cout, cin, code, d.data_ptr(), ops.stream_ptr()), "y3_pack_filter_dgrad")
        assert_bits(f, ref("fwd", case, dtype), f"y3_pack_filter over a sentinel {case}", tf)
        assert_bits(d, ref("dgrad", case, dtype), f"y3_pack_filter_dgrad over a sentinel {case}", td)
        if dtype == torch.float32:
            continue   # the pair is f16 / bf16
        pf, pd = ops.pack_filter_pair(w, cout, cin, dtype)
        assert_bits(pf, ref("fwd", case, dtype), f"pack_filter_pair forward {case}", tf)
        assert_bits(pd, ref("dgrad", case, dtype), f"pack_filter_pair data-gradient {case}", td)
        f.fill_(SENTINEL)
        d.fill_(SENTINEL)
        _lib.check(L.y3_pack_filter_pair(w.data_ptr(), co, ci, k, cout, cin, code, f.data_ptr(), d.data_ptr(), ops.stream_ptr()), "y3_pack_filter_pair")
        assert_bits(f, ref("fwd", case, dtype), f"y3_pack_filter_pair forward over a sentinel {case}", tf)
        assert_bits(d, ref("dgrad", case, dtype), f"y3_pack_filter_pair data-gradient over a sentinel {case}", td)


@pytest.mark.parametrize("dtype", HALVES, ids=["fp16", "bf16"])
def test_stem_and_stride2_banks(dev, dtype):
    from yolov3_amd import _lib, ops

    L, code = _lib.lib(), ops.dtype_code(dtype)
    for case in fb.STEM:
        co, ci, cout = case
        w = fb.weights((co, ci, 3, 3)).to(dev)
        assert_bits(ops.pack_filter_stem(w, cout, dtype), ref("stem", case, dtype), f"pack_filter_stem {case}")
        bank = sentinel_bank(L.y3_packed_filter_stem_elems(cout), dtype, dev)
        _lib.check(L.y3_pack_filter_stem(w.data_ptr(), co, ci, cout, code, bank.data_ptr(), ops.stream_ptr()), "y3_pack_filter_stem")
        assert_bits(bank, ref("stem", case, dtype), f"y3_pack_filter_stem over a sentinel {case}")
    for case in fb.STRIDE2:
        co, ci, cout, cin = case
        w = fb.weights((co, ci, 3, 3)).to(dev)
        bank = sentinel_bank(L.y3_packed_filter_dgrad_s2_elems(cout, cin), dtype, dev)
        _lib.check(L.y3_pack_filter_dgrad_s2(w.data_ptr(), co, ci, cout, cin, code, bank.data_ptr(), ops.stream_ptr()), "y3_pack_filter_dgrad_s2")
        assert_bits(bank, ref("s2", case, dtype), f"y3_pack_filter_dgrad_s2 over a sentinel {case}")


@pytest.mark.parametrize("dtype", HALVES, ids=["fp16", "bf16"])
def test_pack_jobs_table(dev, dtype):
    """one table with every generic case; the Detect head forward-only, the last case data-gradient-only"""
    from yolov3_amd import ops

    jobs = ops.PackJobs(dtype, dev)
    banks = []
    for i, (co, ci, k, cout, cin) in enumerate(fb.GENERIC):
        banks.append(jobs.add(fb.weights((co, ci, k, k)).to(dev), cout, cin, i != len(fb.GENERIC) - 1, i != 3))
    jobs.run()
    torch.cuda.synchronize()
    for i, (case, (f, d)) in enumerate(zip(fb.GENERIC, banks)):
        assert (f is None) == (i == len(fb.GENERIC) - 1) and (d is None) == (i == 3)
        if f is not None:
            assert_bits(f, ref("fwd", case, dtype), f"PackJobs forward {case}")
        if d is not None:
            assert_bits(d, ref("dgrad", case, dtype), f"PackJobs data-gradient {case}")


@pytest.mark.parametrize("dtype", HALVES + [torch.float32], ids=["fp16", "bf16", "fp32"])
def test_fold_pack_jobs_table_without_batchnorm(dev, dtype):
    """w' = w: every generic case and (f16 / bf16, where the stem kernel exists) both stem cases in one table"""
    from yolov3_amd import engine

    def conv_of(co, ci, k):
        conv = nn.Conv2d(ci, co, k, 1, k // 2, bias=False)
        with torch.no_grad():
            conv.weight.copy_(fb.weights((co, ci, k, k)))
        return conv.to(dev)

    jobs = engine.FoldPackJobs(dtype, dev)
    got = [("fwd", case, jobs.add(conv_of(*case[:3]), None, False, cin_pad=case[4])) for case in fb.GENERIC]
    if dtype != torch.float32:
        got += [("stem", case, jobs.add(conv_of(case[0], case[1], 3), None, False, stem=True)) for case in fb.STEM]
    jobs.run()
    torch.cuda.synchronize()
    for kind, case, cw in got:
        assert_bits(cw.filt, ref(kind, case, dtype), f"FoldPackJobs {kind} {case}")
        assert not bool(cw.bias.any())
