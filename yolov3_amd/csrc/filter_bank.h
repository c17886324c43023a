// The packed filter banks: the ONE definition of every layout a packer (filter_bank.hip) writes and a conv kernel reads.  Everything here is
// __host__ __device__: the launch code sizes banks with the same functions the kernels index them with.
//
//   generic bank   [rows][kpad], rows = filters padded to 128, K = (tap, channel) tap-major padded to 64 -- y3_conv2d_fwd and every kernel behind it.  The
//                  data-gradient bank is the same layout with the roles swapped (rows = input channels, K over the filters) and the taps flipped.
//   fragment copy  a second copy behind a generic 3x3 bank with rows % 256 == 0 and channels % 32 == 0, in the order conv_v10.h loads it (y3_frag_index)
//   stride-2 banks four generic data-gradient banks back to back, one per output-parity class, each over its own 1, 2, 2 or 4 taps -- y3_conv2d_dgrad_s2
//   stem bank      [filters padded to 32][kh][kw * 4 + channel], <= 4 channels, the kw = 3 column zero -- stem.hip
#pragma once
#include <stddef.h>

#define Y3_HD __host__ __device__ static inline

// ---- generic bank ---------------------------------------------------------------------------------------------------
Y3_HD int y3_filter_rows(int cout) { return (cout + 127) / 128 * 128; }
Y3_HD int y3_filter_kpad_taps(int ntaps, int channels) { return (ntaps * channels + 63) / 64 * 64; }
Y3_HD int y3_filter_kpad(int cin, int ksize) { return y3_filter_kpad_taps(ksize * ksize, cin); }
// 3x3 banks with rows % 256 == 0 and channels % 32 == 0 carry a second copy behind the row-major one, in the order conv_v10.h consumes it: per
// (256-row filter tile, 64-row wave, K-step) one 4 KiB block of four 1 KiB MFMA A fragments j = 2 kk + a (k-substep kk, rows 32 a .. 32 a + 31), lane = 32 fk + row
// holding k-group 16 kk + 8 fk .. + 7 of the K-step's 32 channels; K-steps in loop order (channel block, tap).  Every packer writes both copies.
Y3_HD bool y3_filter_has_frag(int rows, int channels, int ksize) { return ksize == 3 && rows > 0 && (rows % 256) == 0 && channels > 0 && (channels % 32) == 0; }
Y3_HD long long y3_frag_index(int row, int k, int channels) {
    const int tap = k / channels, ci = k - tap * channels;
    const int cb = ci >> 5, kk = (ci >> 4) & 1, fk = (ci >> 3) & 1, e = ci & 7;
    const int tw = row >> 6, a = (row >> 5) & 1, fr = row & 31;   // tw = 4 * filter tile + wave
    const int nk = 9 * (channels >> 5);
    return ((((long long)tw * nk + cb * 9 + tap) * 4 + (kk * 2 + a)) * 64 + fk * 32 + fr) * 8 + e;
}
Y3_HD size_t y3_filter_elems(int rows, int channels, int ksize) {
    return (size_t)y3_filter_rows(rows) * (size_t)y3_filter_kpad(channels, ksize) * (y3_filter_has_frag(rows, channels, ksize) ? 2 : 1);
}

// ---- stem bank ------------------------------------------------------------------------------------------------------
constexpr int Y3_STEM_KPAD = 48;   // 3 kh x (4 kw slots x 4 channels): a filter row of the image is one 16-element (32-byte) piece per kh
Y3_HD int y3_stem_rows(int cout) { return (cout + 31) / 32 * 32; }
Y3_HD int y3_stem_index(int co, int kh, int kw, int c) { return co * Y3_STEM_KPAD + kh * 16 + kw * 4 + c; }

// ---- stride-2 data gradient -----------------------------------------------------------------------------------------
// The gradient pixels of a 3x3 stride-2 pad-1 conv split into four parity classes (hi % 2, wi % 2) = (ph, pw), class index 2 ph + pw.  Class (ph, pw) only ever
// meets the taps kh = 1 (ph = 0) or kh in {0, 2} (ph = 1), likewise for kw: tap (ih, iw) of the class is source tap (kh[ih], kw[iw]) and reads du at (+dh[ih], +dw[iw]).
struct S2Class {
    int nh, nw;
    int kh[2], dh[2], kw[2], dw[2];
};
Y3_HD S2Class s2_class(int ph, int pw) {
    S2Class c = {};
    if (ph == 0) { c.nh = 1; c.kh[0] = 1; c.dh[0] = 0; } else { c.nh = 2; c.kh[0] = 0; c.dh[0] = 1; c.kh[1] = 2; c.dh[1] = 0; }
    if (pw == 0) { c.nw = 1; c.kw[0] = 1; c.dw[0] = 0; } else { c.nw = 2; c.kw[0] = 0; c.dw[0] = 1; c.kw[1] = 2; c.dw[1] = 0; }
    return c;
}
// the four class banks [rows][kpad[i]] of one layer, back to back: bank i starts at element off[i], `total` elements in all
struct S2Banks {
    int rows, kpad[4];
    size_t off[4], total;
};
Y3_HD S2Banks s2_banks(int cout, int cin) {
    S2Banks g;
    g.rows = y3_filter_rows(cin);
    g.total = 0;
    for (int i = 0; i < 4; ++i) {
        const S2Class c = s2_class(i >> 1, i & 1);
        g.kpad[i] = y3_filter_kpad_taps(c.nh * c.nw, cout);
        g.off[i] = g.total;
        g.total += (size_t)g.rows * g.kpad[i];
    }
    return g;
}

// ---- one description of a destination-indexed bank --------------------------------------------------------------------
// Element (row, k) of the bank [rows][kpad], k = tap * cpt + c, comes from the source tap (kh, kw) that entry `tap` of the tap table names, of the OIHW weights (cout_src, cin_src, ks, ks): of filter
// `row` and channel c, or (row_is_channel) of filter c and channel `row`.  Everything else -- a row or c beyond the source's, a tap without a source, K padding -- is zero.
constexpr int Y3_BANK_MAX_TAPS = 12;
constexpr unsigned Y3_BANK_NO_TAP = 15;
static_assert(4 * Y3_BANK_MAX_TAPS <= 64, "the tap table is one 64-bit word");
struct y3_bank {
    int rows, kpad;
    int row_is_channel;   // 0: forward, stem; 1: the data-gradient banks
    int cpt;              // channels per tap
    int ntaps;
    unsigned long long taps;   // the tap table, 4 bits per tap: kh | kw << 2, or Y3_BANK_NO_TAP (the stem's fourth column) -- a kernel argument the lanes index by shifting, not by loading
    int frag;             // a fragment-ordered copy follows the rows * kpad elements
    int cout_src, cin_src, ks;
};
Y3_HD void y3_bank_set_tap(y3_bank& b, int tap, int kh, int kw) { b.taps |= (unsigned long long)(kh < 0 ? Y3_BANK_NO_TAP : (unsigned)(kh | kw << 2)) << (4 * tap); }
// OIHW offset of bank element (row, k), or -1 for a zero
Y3_HD long long y3_bank_source(const y3_bank& b, int row, int k) {
    const int tap = k / b.cpt, c = k - tap * b.cpt;
    if (tap >= b.ntaps) return -1;
    const unsigned t = (unsigned)(b.taps >> (4 * tap)) & 15u;
    if (t == Y3_BANK_NO_TAP) return -1;
    const int kh = (int)(t & 3u), kw = (int)(t >> 2);
    const int co = b.row_is_channel ? c : row, ci = b.row_is_channel ? row : c;
    if (co >= b.cout_src || ci >= b.cin_src) return -1;
    return (((long long)co * b.cin_src + ci) * b.ks + kh) * b.ks + kw;
}

// the five ways of filling it (ks <= 3 is the caller's to check: kh and kw take two bits each)
Y3_HD y3_bank y3_bank_source_of(int cout_src, int cin_src, int ks) {
    y3_bank b = {};
    b.cout_src = cout_src; b.cin_src = cin_src; b.ks = ks;
    return b;
}
Y3_HD y3_bank y3_bank_fwd(int cout_src, int cin_src, int ks, int cout, int cin) {
    y3_bank b = y3_bank_source_of(cout_src, cin_src, ks);
    b.rows = y3_filter_rows(cout); b.kpad = y3_filter_kpad(cin, ks);
    b.cpt = cin; b.ntaps = ks * ks; b.frag = y3_filter_has_frag(cout, cin, ks);
    for (int t = 0; t < b.ntaps; ++t) y3_bank_set_tap(b, t, t / ks, t % ks);
    return b;
}
// the data-gradient convolution has `cin` filters of ks * ks * cout taps: the same geometry with the roles swapped, taps flipped
Y3_HD y3_bank y3_bank_dgrad(int cout_src, int cin_src, int ks, int cout, int cin) {
    y3_bank b = y3_bank_source_of(cout_src, cin_src, ks);
    b.rows = y3_filter_rows(cin); b.kpad = y3_filter_kpad(cout, ks);
    b.row_is_channel = 1; b.cpt = cout; b.ntaps = ks * ks; b.frag = y3_filter_has_frag(cin, cout, ks);
    for (int t = 0; t < b.ntaps; ++t) y3_bank_set_tap(b, t, ks - 1 - t / ks, ks - 1 - t % ks);
    return b;
}
Y3_HD y3_bank y3_bank_dgrad_s2(int cout_src, int cin_src, int cout, int cin, int cls) {
    const S2Class c = s2_class(cls >> 1, cls & 1);
    y3_bank b = y3_bank_source_of(cout_src, cin_src, 3);
    b.rows = y3_filter_rows(cin); b.kpad = y3_filter_kpad_taps(c.nh * c.nw, cout);
    b.row_is_channel = 1; b.cpt = cout; b.ntaps = c.nh * c.nw;
    for (int t = 0; t < b.ntaps; ++t) y3_bank_set_tap(b, t, c.kh[t / c.nw], c.kw[t % c.nw]);
    return b;
}
Y3_HD y3_bank y3_bank_stem(int cout_src, int cin_src, int cout) {
    y3_bank b = y3_bank_source_of(cout_src, cin_src, 3);
    b.rows = y3_stem_rows(cout); b.kpad = Y3_STEM_KPAD;
    b.cpt = 4; b.ntaps = 12;   // tap = kh * 4 + kw slot
    for (int t = 0; t < 12; ++t) y3_bank_set_tap(b, t, (t & 3) < 3 ? t >> 2 : -1, t & 3);
    return b;
}
