"""Shared cases of the filter-bank tests (tests/test_filter_bank_cpu.py, tests/test_gpu_filter_bank.py) and a plain torch restatement of the four bank layouts
(yolov3_amd/csrc/filter_bank.h) in this project's own words: an fp32 OIHW tensor is permuted / flipped into zeros, then rounded with .to(dtype).  Nothing here calls
the library.  Not a test file."""
from __future__ import annotations

import torch

# (cout_src, cin_src, k, cout, cin): the smallest shapes at which each thing can go wrong
GENERIC = [
    (21, 8, 3, 24, 8),       # row padding 24 -> 128, K 72 -> 128, a ragged source tile in both directions
    (40, 40, 1, 40, 40),     # two source tiles per axis, the second 8 wide; K 40 -> 64
    (64, 3, 3, 64, 8),       # channel padding of the generic layer-0 form
    (255, 64, 1, 256, 64),   # a Detect head
    (256, 32, 3, 256, 32),   # the smallest forward fragment copy, behind a K-padded row-major part (288 -> 320)
    (32, 256, 3, 32, 256),   # the smallest data-gradient fragment copy (rows = cin)
    (128, 64, 3, 128, 64),   # 3x3 without a second copy
]
STEM = [(32, 3, 32), (64, 4, 64)]                      # (cout_src, cin_src, cout)
STRIDE2 = [(64, 32, 64, 32), (21, 40, 24, 40)]         # (cout_src, cin_src, cout, cin): class banks, with padding in the second


def weights(shape, seed=11):
    """seeded fp32 weights, never modified"""
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def rows_of(n: int) -> int:
    return -(-n // 128) * 128


def kpad_of(n: int) -> int:
    return -(-n // 64) * 64


def has_frag(rows: int, channels: int, k: int) -> bool:
    return k == 3 and rows > 0 and rows % 256 == 0 and channels > 0 and channels % 32 == 0


def frag_tail(rows: int, channels: int, k: int) -> int:
    """elements at the end of a bank that nothing writes and nothing reads: the fragment-ordered copy holds rows * 9 * channels elements of the rows * kpad behind the
    row-major part (the zero-filled banks of the job launches hold zeros there, a bank of the single-layer packers what it held before)"""
    return rows_of(rows) * (kpad_of(9 * channels) - 9 * channels) if has_frag(rows, channels, k) else 0


def _generic(t: torch.Tensor, rows: int, channels: int, k: int) -> torch.Tensor:
    """t (rows_src, taps, channels_src) fp32 -> [rows pad 128][taps * channels pad 64] (+ the fragment-ordered copy, zeros in its unwritten tail)"""
    r_src, taps, c_src = t.shape
    nr, kp = rows_of(rows), kpad_of(taps * channels)
    std = torch.zeros(nr, taps, channels)
    std[:r_src, :, :c_src] = t
    bank = torch.zeros(nr, kp)
    bank[:, : taps * channels] = std.reshape(nr, taps * channels)
    if not has_frag(rows, channels, k):
        return bank.reshape(-1)
    # [tile-wave][a][row][tap][cb][kk][fk][e] -> [tile-wave][K-step = 9 cb + tap][kk][a][fk][row][e]
    frag = std.view(rows // 64, 2, 32, 9, channels // 32, 2, 2, 8).permute(0, 4, 3, 5, 1, 6, 2, 7).reshape(-1)
    return torch.cat([bank.reshape(-1), frag, torch.zeros(nr * kp - frag.numel())])


def ref_fwd(w: torch.Tensor, cout: int, cin: int, dtype) -> torch.Tensor:
    """forward bank: rows = filters, K = (kh, kw, channel)"""
    co, ci, k, _ = w.shape
    return _generic(w.permute(0, 2, 3, 1).reshape(co, k * k, ci), cout, cin, k).to(dtype)


def ref_dgrad(w: torch.Tensor, cout: int, cin: int, dtype) -> torch.Tensor:
    """data-gradient bank: rows = channels, K = (flipped kh, flipped kw, filter)"""
    co, ci, k, _ = w.shape
    return _generic(w.flip(2, 3).permute(1, 2, 3, 0).reshape(ci, k * k, co), cin, cout, k).to(dtype)


def ref_dgrad_s2(w: torch.Tensor, cout: int, cin: int, dtype) -> torch.Tensor:
    """the four parity-class banks (ph, pw) = (0,0), (0,1), (1,0), (1,1) back to back: class taps kh = 1 (ph = 0) or kh in (0, 2) (ph = 1), likewise kw; not flipped"""
    co, ci, k, _ = w.shape
    assert k == 3
    banks = []
    for ph in (0, 1):
        for pw in (0, 1):
            khs, kws = ([1], [0, 2])[ph], ([1], [0, 2])[pw]
            sub = w[:, :, khs][:, :, :, kws]   # (co, ci, nh, nw)
            banks.append(_generic(sub.permute(1, 2, 3, 0).reshape(ci, len(khs) * len(kws), co), cin, cout, 0))
    return torch.cat(banks).to(dtype)


def ref_stem(w: torch.Tensor, cout: int, dtype) -> torch.Tensor:
    """[filters pad 32][kh][kw * 4 + channel], the kw = 3 column and the channels beyond the source's zero"""
    co, ci, k, _ = w.shape
    assert k == 3 and ci <= 4
    bank = torch.zeros(-(-cout // 32) * 32, 3, 4, 4)
    bank[:co, :, :3, :ci] = w.permute(0, 2, 3, 1)
    return bank.reshape(-1).to(dtype)
