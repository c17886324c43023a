// Fused Conv2d + bias + SiLU (+ residual, + nearest-x2 scatter, + channel-slice write) for gfx950.
//
// Replaces reference models/common.py:75/:81 (Conv.forward / forward_fuse), :165 (Bottleneck add),
// models/yolov3.yaml:43,51 (nn.Upsample) and models/common.py:428 (torch.cat) -- see include/yolov3_hip.h.
//
// Formulation: implicit GEMM, D[cout][pixel] = sum_k W[cout][k] * X[pixel][k], k = (kh, kw, cin).
//   * activations NHWC, filters packed [cout][kh][kw][cin]: BOTH operands are K-contiguous, so a lane's
//     16-byte load is exactly the 8-element k-group an MFMA fragment wants.
//   * v_mfma_f32_32x32x16_{f16,bf16}: A operand = filters (rows = cout), B operand = pixels (cols),
//     so each lane ends up holding 4 consecutive couts of ONE pixel per register quad -> NHWC friendly.
//   * 256 threads = 4 waves; tile TC couts x TP pixels x BK; register-staged global->LDS with XOR-swizzled
//     16-byte slots (conflict-free ds_read_b128 fragment reads), double-buffered LDS, one barrier / K-step.
//   * epilogue: bias + SiLU in registers, fp32 tile through LDS, then fully coalesced 16-byte row stores
//     with the residual added on the way out (single rounding).
//   * grid: 1-D, XCD-aware (block b runs on XCD b%8): each XCD owns a contiguous range of pixel tiles and
//     walks all cout tiles of a pixel tile back-to-back, so the X tile is L2-hot for its siblings.
#include "y3_common.h"

#include <stdlib.h>
#include <type_traits>
#include <utility>
#include <string.h>

namespace {

struct ConvArgs {
    const void* x;
    const void* w;
    const float* bias;
    const void* res;
    void* y;
    int N, H, W, Cin, xpitch;  // input
    int Ho, Wo, Cout, ypitch;  // output (Ho, Wo are the conv output dims, before any upsample scatter)
    int rpitch;
    int ks, stride, pad;
    int act, ups;
    int dil_shift;  // 0: plain conv; 1: the input is a virtual zero-interleaved (x2) image (stride-2 dgrad)
    int M;          // N*Ho*Wo
    int Kpad;       // packed filter row length (elements)
    int nk;         // K iterations
    int cin_blocks; // Cin / BK (uniform-tap path)
    int n_pt, n_ct;
    unsigned x_bytes, w_bytes;  // extents for the buffer descriptors (0 = tensor beyond 2 GiB: the MFMA path refuses it)
    unsigned y_bytes, r_bytes;  // output / residual extents (the LDS-DMA kernels store through bounds-checked descriptors)
    // multiply-shift reciprocals of Ho*Wo, Wo and n_ct (host: set_divisors): q = n / d for 0 <= n < 2^31 as umulhi(n, mul) >> (sh - 1); mul == 0 means d == 1
    unsigned dv_hw_mul, dv_hw_sh, dv_w_mul, dv_w_sh, dv_ct_mul, dv_ct_sh;
    // tap table: input row/col offset of K-loop tap t is (hi0 + tdh[t], wi0 + tdw[t]) with hi0 = ho*stride - pad.
    // A plain k x k conv lists (kh, kw); the parity classes of a stride-2 data gradient list 1, 2 or 4 taps.
    int ntaps;
    signed char tdh[12], tdw[12];
    unsigned long long tap_lo, tap_hi;   // the same table packed for scalar extraction: tap t -> byte t, (dh + 8) | (dw + 8) << 4  (host: pack_taps)
    // output addressing: conv pixel (n, ho, wo) lands at (n, ho*omul + ooh, wo*omul + oow) of an (oH, oW) image
    int oH, oW, omul, ooh, oow;
    // BatchNorm statistics of the output, taken in the epilogue (training forward): every wave writes the per-filter (sum, sum of
    // squares) of the <= MP*32 pixels it owns -- of the values as STORED (rounded to T) -- into row (pixel tile * stat_wp + its
    // pixel-wave index) of `stats` ([rows][Cout][2] fp32); a fixed-order fp64 sum over the rows follows (train.hip)
    float* stats;
    int stat_wp;   // waves along the pixel axis of the launched variant
    void* ws;      // the caller's scratch (y3_conv2d_fwd_ws): fp32 slabs of the K-split form of conv_v10.h; may be null
    size_t ws_bytes;
    int v10_S;     // conv_v10.h SPLIT form: slices of the channel blocks
    unsigned dv_sl_mul, dv_sl_sh;   // reciprocal of the blocks per slice
    int v10_B, v10_q, v10_r, v10_nt_hi, v10_nt_lo;   // conv_v10.h: blocks per filter tile, 32-pixel column blocks per block (+ 1 for the first r), tiles per block for the two run lengths
    int v10_tq_h, v10_tr_h, v10_tq_l, v10_tr_l;      // ... a run of q + 1 / q column blocks as nt_hi / nt_lo tiles of tq (+ 1 for the first tr) column blocks
    int v10_g;                                       // ... blocks per interleave group (the blocks of a filter tile that share an XCD); 1 = every block walks its own contiguous run
    unsigned dv_g_mul, dv_g_sh;                      // reciprocal of v10_g
    int cs_strips, cs_T, cs_per;   // conv_strip.h: column strips per row, output rows in all, output rows per block
    unsigned dv_pw_mul, dv_pw_sh, dv_h1_mul, dv_h1_sh;   // conv_v10.h: reciprocals of W + 2 and H + 1
    // conv_1x1s.h, input transform (training forward): x is the producing layer's pre-BatchNorm tensor u; the operand is y_in = act(in_scale u + in_shift) (+ in_res), stored to in_y
    const float* in_scale;
    const float* in_shift;
    const void* in_res;
    void* in_y;
    int in_rpitch, in_ypitch, in_act;
    unsigned in_r_bytes, in_y_bytes;
#ifdef Y3_TIMELINE  // debug build only (tools/timeline.py): per-block wall-clock stamps
    unsigned long long* tl;
#endif
};
#ifdef Y3_TIMELINE
static unsigned long long* g_timeline = nullptr;
#define Y3_STAMP(i) do { if (p.tl && threadIdx.x == 0) p.tl[(long long)blockIdx.x * 8 + (i)] = wall_clock64(); } while (0)
#else
#define Y3_STAMP(i) do { } while (0)
#endif

static thread_local const char* g_last_variant = "";   // kernel variant of the last launch on this thread (y3_conv_last_variant); written by launch_begin and the two quad launches only

template <typename T> struct Mfma;
template <> struct Mfma<f16_t> {
    typedef f16x8 frag;
    static Y3_DEV f32x16 run(frag a, frag b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0); }
};
template <> struct Mfma<bf16_t> {
    typedef bf16x8 frag;
    static Y3_DEV f32x16 run(frag a, frag b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0); }
};

template <int BK> Y3_DEV int swz(int row) {
    constexpr int S = BK / 8;   // 16-byte slots per row
    constexpr int R = 16 / S;   // rows per 256-byte LDS line
    return (row / R) % S;
}

// forced tile variant for A/B runs (knob "conv", y3_common.h); 3 = per-shape dispatch
static int conv_variant() {
    const int v = (int)y3_knob(Y3K_CONV);
    return v == 0 ? 3 : v;
}

Y3_DEV int fdiv(int n, unsigned mul, unsigned sh) { return mul ? (int)(__umulhi((unsigned)n, mul) >> (sh - 1)) : n; }
// output pixel m -> (image, row, column)
Y3_DEV void pix_coords(int m, const ConvArgs& p, int& n, int& ho, int& wo) {
    n = fdiv(m, p.dv_hw_mul, p.dv_hw_sh);
    const int rem = m - n * (p.Ho * p.Wo);
    ho = fdiv(rem, p.dv_w_mul, p.dv_w_sh);
    wo = rem - ho * p.Wo;
}
static void magic_u31(int d, unsigned& mul, unsigned& sh) {   // host side of fdiv
    if (d <= 1) { mul = 0; sh = 1; return; }
    unsigned s = 0;
    while ((1ll << s) < d) ++s;
    mul = (unsigned)(((1ull << (31 + s)) / (unsigned long long)d) + 1ull);
    sh = s;
}
static void pack_taps(ConvArgs& a) {
    a.tap_lo = a.tap_hi = 0;
    for (int t = 0; t < a.ntaps; ++t) {
        const unsigned long long b = (unsigned long long)((a.tdh[t] + 8) & 15) | ((unsigned long long)((a.tdw[t] + 8) & 15) << 4);
        if (t < 8) a.tap_lo |= b << (8 * t); else a.tap_hi |= b << (8 * (t - 8));
    }
}
// (dh, dw) of tap t from the packed table; t is wave-uniform, so this stays on the scalar unit (indexing tdh[]/tdw[] with a
// run-time tap costs a vector load from the kernarg segment in front of every K-step's gather)
Y3_DEV void tap_offsets(const ConvArgs& p, int t, int& dh, int& dw) {
    const unsigned long long w = t < 8 ? p.tap_lo >> (8 * t) : p.tap_hi >> (8 * (t - 8));
    dh = (int)(w & 15) - 8;
    dw = (int)((w >> 4) & 15) - 8;
}
static void set_divisors(ConvArgs& a) {
    pack_taps(a);
    magic_u31(a.Ho * a.Wo, a.dv_hw_mul, a.dv_hw_sh);
    magic_u31(a.Wo, a.dv_w_mul, a.dv_w_sh);
    magic_u31(a.n_ct, a.dv_ct_mul, a.dv_ct_sh);
}

Y3_DEV long long out_pix(int n, int ho, int wo, const ConvArgs& p) {
    return (long long)(n * p.oH + ho * p.omul + p.ooh) * p.oW + wo * p.omul + p.oow;
}

// Gather helpers shared by the MFMA kernels.  (hi, wi) are coordinates in the (virtually dilated) input image.
Y3_DEV bool in_image(int hi, int wi, const ConvArgs& p) {
    const int msk = (1 << p.dil_shift) - 1;
    return (int)(((hi | wi) & msk) == 0) & (int)((unsigned)(hi >> p.dil_shift) < (unsigned)p.H) & (int)((unsigned)(wi >> p.dil_shift) < (unsigned)p.W);
}
Y3_DEV int tap_bytes(int hi0, int wi0, int kh, int kw, int c0, const ConvArgs& p) {
    const int hi = (hi0 + kh) >> p.dil_shift, wi = (wi0 + kw) >> p.dil_shift;
    return ((hi * p.W + wi) * p.xpitch + c0) * 2;
}

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// ---- epilogue of the MFMA kernels: per-wave transpose through LDS ---------------------------------------------------------
// A 32x32 MFMA tile leaves lane (pixel = lane & 31, fk = lane >> 5) with filters 8g + 4fk + q (g, q < 4) of that pixel.
// All waves apply bias + SiLU to their own accumulators at once; one v_permlane32_swap per register pair then gives every lane
// 8 CONSECUTIVE filters of its pixel, which it rounds to T and drops as one 16-byte chunk into the wave's PRIVATE slice of
// the (now idle) stage buffers, laid out [pixel][MC*32 filters] with the K-loop's XOR chunk swizzle.  Reading the slice back
// row-major gives each store instruction whole MC*64-byte runs of a pixel's NHWC row; the residual rows are fetched with
// the same coalesced pattern before the arithmetic starts and added in fp32.  One block barrier (the stage buffers must be
// idle), no idle waves.  (The block-wide fp32 transpose this replaces cost 8-17 us per block with half of the waves parked
// during the exp/rcp pass; a register-only variant with 32-byte runs lost on the residual layers: profiles/r01_conv_timeline.md.)
// STAT_ACC (conv_strip.h: a wave calls this once per output row of its strip): the statistics are added to the caller's 16 registers `sacc` (8 sums, 8 sums of
// squares of the lane's 8 filters) instead of being written; epilogue_stats_flush writes ONE row for all the calls.
// IDENT (conv_v10.h: stride 1, no upsample scatter, no parity-class output): the output pixel index IS the GEMM column m, so the lane's store offsets are plain
// arithmetic on m -- no (image, row, column) decomposition, no 64-bit products, no ds_bpermute from the MFMA layout to the store layout.
template <typename T, int MC, int MP, bool STAT_ACC = false, bool IDENT = false>
Y3_DEV void epilogue_wave(const ConvArgs& p, f32x16 (&acc)[MC][MP], unsigned char* wl, int c_base, int m_base, int lane, int stat_row = -1, int m_end = 0x7fffffff,
                          float* sacc = nullptr) {
    typedef typename Mfma<T>::frag vec8;   // 8 x T = one 16-byte chunk
    constexpr int CH = MC * 4;          // 16-byte chunks per pixel row of this wave's slice
    constexpr int RB = CH * 16;         // row bytes
    constexpr int PPI = 64 / CH;        // pixels per load/store instruction
    constexpr int NI = MP * 32 / PPI;   // instructions per lane
    constexpr unsigned OOB = 0xffffffffu;
    const int frow = lane & 31, fk = lane >> 5;
    const int rp = lane / CH, ch = lane % CH;
    const bool has_res = p.res != nullptr;
    // bounds-checked descriptors: lanes beyond M / Cout carry offset 0xffffffff (loads return 0, stores are dropped)
    const auto rsrc_y = __builtin_amdgcn_make_buffer_rsrc((void*)p.y, 0, (int)p.y_bytes, 0x00020000);
    const auto rsrc_r = __builtin_amdgcn_make_buffer_rsrc((void*)(has_res ? p.res : p.y), 0, has_res ? (int)p.r_bytes : 0, 0x00020000);

    // output pixel index of the MFMA pixels this lane owns (-1: beyond M or beyond the tile's valid pixels), then re-distributed to the store layout
    const int mlim = m_end < p.M ? m_end : p.M;
    int opx[MP];
    if constexpr (!IDENT) {
#pragma unroll
        for (int b = 0; b < MP; ++b) {
            const int m = m_base + b * 32 + frow;
            const int mm = m < mlim ? m : 0;
            int n, ho, wo;
            pix_coords(mm, p, n, ho, wo);
            const int o = p.ups ? ((n * p.Ho * 2 + 2 * ho) * (p.Wo * 2) + 2 * wo) : (int)out_pix(n, ho, wo, p);
            opx[b] = m < mlim ? o : -1;
        }
    }
    const int c = c_base + ch * 8;
    const bool cv = c + 8 <= p.Cout;
    unsigned yoff[NI];
    u32x4 rres[NI];
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        const int pl = i * PPI + rp;    // pixel (row of the slice) this lane stores in step i
        int spx;
        if constexpr (IDENT) {
            const int m = m_base + pl;
            spx = m < mlim ? m : -1;
        } else {
            spx = __builtin_amdgcn_ds_bpermute((pl & 31) << 2, opx[(i * PPI) / 32]);
        }
        const bool ok = cv && spx >= 0;
        yoff[i] = ok ? (unsigned)(spx * p.ypitch + c) * 2u : OOB;
        if constexpr (!IDENT) {
            if (has_res) rres[i] = __builtin_amdgcn_raw_buffer_load_b128(rsrc_r, ok ? (unsigned)(spx * p.rpitch + c) * 2u : OOB, 0, 0);
        }
    }
    if constexpr (IDENT) {   // (one uniform branch around the eight loads instead of one per load)
        if (has_res) {
#pragma unroll
            for (int i = 0; i < NI; ++i) {
                const int m = m_base + i * PPI + rp;
                rres[i] = __builtin_amdgcn_raw_buffer_load_b128(rsrc_r, yoff[i] != OOB ? (unsigned)(m * p.rpitch + c) * 2u : OOB, 0, 0);
            }
        }
    }

    // activation on whole accumulators (straight-line transcendentals + packed fp32, y3_common.h), pairs of consecutive filters rounded to T
    // by one v_cvt_pk each, THEN the halves of the packed registers swapped between the lane halves: per accumulator 8 conversions and
    // 8 swaps instead of 16 + 16 + 8 packs (the epilogue is VALU work in series with the block's K loop)
    auto stash = [&](auto silu) {
#pragma unroll
        for (int a = 0; a < MC; ++a)
#pragma unroll
            for (int b = 0; b < MP; ++b)
#pragma unroll
                for (int gp = 0; gp < 2; ++gp) {
                    f32x8 v;   // filters 16gp + 4fk + (0..3) and 16gp + 8 + 4fk + (0..3)
#pragma unroll
                    for (int q = 0; q < 8; ++q) v[q] = acc[a][b][8 * gp + q];
                    if (decltype(silu)::value) silu_vec<f32x8, 8>(v);
                    u32x4 ov;
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        const auto sw = __builtin_amdgcn_permlane32_swap(pack2<T>(v[2 * h], v[2 * h + 1]), pack2<T>(v[4 + 2 * h], v[4 + 2 * h + 1]), false, false);
                        ov[h] = (unsigned)sw[0];
                        ov[2 + h] = (unsigned)sw[1];
                    }
                    const int pl = b * 32 + frow;
                    const int chunk = a * 4 + gp * 2 + fk;
                    *(u32x4*)(wl + pl * RB + ((chunk ^ swz<MC * 32>(pl)) << 4)) = ov;
                    __builtin_amdgcn_sched_barrier(0);   // eight values at a time: the temporaries stay at 8 registers
                }
    };
    if (p.act == Y3_ACT_SILU) stash(std::true_type{}); else stash(std::false_type{});
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const bool want_stats = p.stats != nullptr;   // kernel-uniform
    float st0[8], st1[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) { st0[q] = STAT_ACC ? sacc[q] : 0.0f; st1[q] = STAT_ACC ? sacc[8 + q] : 0.0f; }
    // the read-back / store loop, one straight-line copy per kernel-uniform case (written with the tests inside the loop the compiler kept a branch per store:
    // ~25 scalar branches and their mask arithmetic per pass)
    auto drain = [&](auto STATS, auto RES, auto UPS) {
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const int pl = i * PPI + rp;
            vec8 ov = *(const vec8*)(wl + pl * RB + ((ch ^ swz<MC * 32>(pl)) << 4));
            if constexpr (decltype(STATS)::value) {   // (select, not a divergent branch: pixels beyond the tile / the tensor count as zeros)
                const bool live = yoff[i] != OOB;
#pragma unroll
                for (int q = 0; q < 8; ++q) { const float f = live ? to_f32<T>(ov[q]) : 0.0f; st0[q] += f; st1[q] += f * f; }
            }
            if constexpr (decltype(RES)::value) {   // x + cv2(cv1(x)) in fp32, rounded once (what torch's half add does)
                const vec8 rr = __builtin_bit_cast(vec8, rres[i]);
                u32x4 sum;
#pragma unroll
                for (int q = 0; q < 8; q += 2) sum[q >> 1] = pack2<T>(to_f32<T>(ov[q]) + to_f32<T>(rr[q]), to_f32<T>(ov[q + 1]) + to_f32<T>(rr[q + 1]));
                ov = __builtin_bit_cast(vec8, sum);
            }
            const u32x4 raw = __builtin_bit_cast(u32x4, ov);
            if constexpr (!decltype(UPS)::value) {
                __builtin_amdgcn_raw_buffer_store_b128(raw, rsrc_y, yoff[i], 0, 0);
            } else {
#pragma unroll
                for (int dy = 0; dy < 2; ++dy)
#pragma unroll
                    for (int dx = 0; dx < 2; ++dx)
                        __builtin_amdgcn_raw_buffer_store_b128(raw, rsrc_y, yoff[i] == OOB ? OOB : yoff[i] + (unsigned)((dy * p.Wo * 2 + dx) * p.ypitch) * 2u, 0, 0);
            }
        }
    };
    if (!IDENT && p.ups) drain(std::false_type{}, std::false_type{}, std::true_type{});   // (the scatter form takes neither a residual nor statistics: conv_fwd_impl)
    else if (want_stats) { if (has_res) drain(std::true_type{}, std::true_type{}, std::false_type{}); else drain(std::true_type{}, std::false_type{}, std::false_type{}); }
    else if (has_res) drain(std::false_type{}, std::true_type{}, std::false_type{});
    else drain(std::false_type{}, std::false_type{}, std::false_type{});
    if constexpr (STAT_ACC) {
#pragma unroll
        for (int q = 0; q < 8; ++q) { sacc[q] = st0[q]; sacc[8 + q] = st1[q]; }
    } else if (want_stats) {
        // lanes rp * CH + ch (rp < PPI) hold partial sums of the same 8 filters: butterfly over the rp bits, lane ch writes the row
#pragma unroll
        for (int off = CH; off < 64; off <<= 1)
#pragma unroll
            for (int q = 0; q < 8; ++q) { st0[q] += __shfl_xor(st0[q], off, 64); st1[q] += __shfl_xor(st1[q], off, 64); }
        if (rp == 0 && cv) {
            float* row = p.stats + ((long long)stat_row * p.Cout + c) * 2;
#pragma unroll
            for (int q = 0; q < 8; q += 2) *(f32x4*)(row + q * 2) = f32x4{st0[q], st1[q], st0[q + 1], st1[q + 1]};
        }
    }
}

// the row write of epilogue_wave<.., STAT_ACC = true>: `sacc` as that call left it, MC = the filter tiles of the wave (same lane -> filter mapping)
template <int MC> Y3_DEV void epilogue_stats_flush(const ConvArgs& p, float* sacc, int c_base, int lane, int stat_row) {
    constexpr int CH = MC * 4;
    const int rp = lane / CH, ch = lane % CH;
    const int c = c_base + ch * 8;
#pragma unroll
    for (int off = CH; off < 64; off <<= 1)
#pragma unroll
        for (int q = 0; q < 16; ++q) sacc[q] += __shfl_xor(sacc[q], off, 64);
    if (rp == 0 && c + 8 <= p.Cout) {
        float* row = p.stats + ((long long)stat_row * p.Cout + c) * 2;
#pragma unroll
        for (int q = 0; q < 8; q += 2) *(f32x4*)(row + q * 2) = f32x4{sacc[q], sacc[8 + q], sacc[q + 1], sacc[8 + q + 1]};
    }
}

// ---- v2 main loop: branch-free buffer loads (out-of-range lanes read 0 through the descriptor's bounds check, so
// halo / tail handling costs one v_cndmask instead of a divergent branch) and a two-deep register prefetch: while
// tile t is multiplied out of LDS, tile t+1 waits in registers and tile t+2 is in flight, so a K-step never
// stalls on HBM/L2 latency.  The compiler's counted vmcnt keeps the younger batch in flight across the LDS store.

template <typename T, int BK, int WAVES_C, int WAVES_P, int MC, int MP, bool SMALLC>
__global__ __launch_bounds__(256, 2) void conv_igemm_v2_kernel(const ConvArgs p) {
    constexpr int TC = WAVES_C * MC * 32;
    constexpr int TP = WAVES_P * MP * 32;
    constexpr int S = BK / 8;
    constexpr int WJ = (TC * S + 255) / 256;
    constexpr int XJ = (TP * S + 255) / 256;
    constexpr int STAGE_BYTES = (TC + TP) * BK * 2;
    constexpr int LDS_BYTES = 2 * STAGE_BYTES > TC * TP * 2 ? 2 * STAGE_BYTES : TC * TP * 2;  // K-loop stages, re-used as the epilogue's T-typed output tile
    constexpr int ROWSTEP = 256 / S;
    constexpr bool W_FULL = (TC * S) % 256 == 0, X_FULL = (TP * S) % 256 == 0;  // no partial last chunk -> no row guards
    static_assert(WAVES_C * WAVES_P == 4, "4 waves");
    typedef typename Mfma<T>::frag frag;

    __shared__ __attribute__((aligned(16))) unsigned char smem[LDS_BYTES];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wv = tid >> 6;
    const int wc = wv / WAVES_P, wp = wv % WAVES_P;

    const int L = xcd_remap(blockIdx.x, gridDim.x);
    const int pt = fdiv(L, p.dv_ct_mul, p.dv_ct_sh), ct = L - pt * p.n_ct;

    const auto rsrc_x = __builtin_amdgcn_make_buffer_rsrc((void*)p.x, 0, (int)p.x_bytes, 0x00020000);
    const auto rsrc_w = __builtin_amdgcn_make_buffer_rsrc((void*)p.w, 0, (int)p.w_bytes, 0x00020000);
    constexpr unsigned OOB = 0xffffffffu;

    const int slot = tid % S;
    const int row0 = tid / S;

    int xoff[XJ];  // byte offset of (n, hi0, wi0, 0); may be negative, only used when the tap is inside the image
    int hi0[XJ], wi0[XJ];
    bool mvalid[XJ];
#pragma unroll
    for (int j = 0; j < XJ; ++j) {
        const int row = row0 + j * ROWSTEP;
        const int m = pt * TP + row;
        const bool v = (X_FULL || row < TP) && (m < p.M);
        const int mm = v ? m : 0;
        int n, ho, wo;
        pix_coords(mm, p, n, ho, wo);
        hi0[j] = ho * p.stride - p.pad;
        wi0[j] = wo * p.stride - p.pad;
        xoff[j] = (int)(((long long)n * p.H * p.W * p.xpitch) * 2);  // byte offset of image n
        mvalid[j] = v;
    }
    unsigned woff[WJ];
#pragma unroll
    for (int j = 0; j < WJ; ++j) {
        const int row = row0 + j * ROWSTEP;
        woff[j] = (W_FULL || row < TC) ? (unsigned)(((long long)(ct * TC + row) * p.Kpad + slot * 8) * 2) : OOB;
    }

    u32x4 xa[XJ], wa[WJ], xb[XJ], wb[WJ];

    int nx_tap = 0, nx_cb = 0, nx_kh, nx_kw;
    tap_offsets(p, 0, nx_kh, nx_kw);
    auto issue = [&](int it, u32x4 (&xr)[XJ], u32x4 (&wr)[WJ]) {
        int kh, kw, c0;
        bool tapok = it < p.nk;
        if (SMALLC) {
            const int cg = p.Cin >> 3;
            const int g = it * S + slot;
            const int tap = g / cg;
            c0 = (g - tap * cg) * 8;
            tapok = tapok && (tap < p.ntaps);
            tap_offsets(p, tapok ? tap : 0, kh, kw);
        } else {
            const int cb = nx_cb;   // K-steps are requested strictly in order
            kh = nx_kh; kw = nx_kw;
            if (++nx_cb == p.cin_blocks) { nx_cb = 0; ++nx_tap; tap_offsets(p, nx_tap < p.ntaps ? nx_tap : 0, nx_kh, nx_kw); }
            c0 = cb * BK + slot * 8;
        }
#pragma unroll
        for (int j = 0; j < XJ; ++j) {
            const int hi = hi0[j] + kh, wi = wi0[j] + kw;
            const bool ok = (int)tapok & (int)mvalid[j] & (int)in_image(hi, wi, p);
            xr[j] = __builtin_amdgcn_raw_buffer_load_b128(rsrc_x, ok ? (unsigned)(xoff[j] + tap_bytes(hi0[j], wi0[j], kh, kw, c0, p)) : OOB, 0, 0);
        }
        const unsigned wk = it < p.nk ? (unsigned)(it * BK * 2) : OOB;
#pragma unroll
        for (int j = 0; j < WJ; ++j) wr[j] = __builtin_amdgcn_raw_buffer_load_b128(rsrc_w, (woff[j] == OOB || wk == OOB) ? OOB : woff[j] + wk, 0, 0);
    };
    auto stash = [&](int stage, const u32x4 (&xr)[XJ], const u32x4 (&wr)[WJ]) {
        unsigned char* wl = smem + stage * STAGE_BYTES;
        unsigned char* xl = wl + TC * BK * 2;
#pragma unroll
        for (int j = 0; j < WJ; ++j) {
            const int row = row0 + j * ROWSTEP;
            if (W_FULL || row < TC) *(u32x4*)(wl + row * (BK * 2) + ((slot ^ swz<BK>(row)) << 4)) = wr[j];
        }
#pragma unroll
        for (int j = 0; j < XJ; ++j) {
            const int row = row0 + j * ROWSTEP;
            if (X_FULL || row < TP) *(u32x4*)(xl + row * (BK * 2) + ((slot ^ swz<BK>(row)) << 4)) = xr[j];
        }
    };

    const int frow = lane & 31;
    const int fk = lane >> 5;

    f32x16 acc[MC][MP];   // start at the bias of the lane's filters (see epilogue_wave)
#pragma unroll
    for (int a = 0; a < MC; ++a)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int cb = ct * TC + (wc * MC + a) * 32 + 8 * g + 4 * fk;
            f32x4 bz = {0.f, 0.f, 0.f, 0.f};
            if (p.bias && cb + 4 <= p.Cout) bz = *(const f32x4*)(p.bias + cb);
#pragma unroll
            for (int b = 0; b < MP; ++b)
#pragma unroll
                for (int q = 0; q < 4; ++q) acc[a][b][4 * g + q] = bz[q];
        }

    auto compute = [&](int stage) {
        const unsigned char* wl = smem + stage * STAGE_BYTES;
        const unsigned char* xl = wl + TC * BK * 2;
#pragma unroll
        for (int kk = 0; kk < BK / 16; ++kk) {
            frag af[MC], bf[MP];
            const int ks = kk * 2 + fk;
#pragma unroll
            for (int a = 0; a < MC; ++a) {
                const int row = (wc * MC + a) * 32 + frow;
                af[a] = *(const frag*)(wl + row * (BK * 2) + ((ks ^ swz<BK>(row)) << 4));
            }
#pragma unroll
            for (int b = 0; b < MP; ++b) {
                const int row = (wp * MP + b) * 32 + frow;
                bf[b] = *(const frag*)(xl + row * (BK * 2) + ((ks ^ swz<BK>(row)) << 4));
            }
#pragma unroll
            for (int a = 0; a < MC; ++a)
#pragma unroll
                for (int b = 0; b < MP; ++b) acc[a][b] = Mfma<T>::run(af[a], bf[b], acc[a][b]);
        }
    };

    issue(0, xa, wa);
    issue(1, xb, wb);
    stash(0, xa, wa);
    __syncthreads();
    for (int it = 0; it < p.nk; it += 2) {
        issue(it + 2, xa, wa);       // tile it+2 -> A (in flight during two K-steps)
        compute(0);                  // tile it
        stash(1, xb, wb);            // tile it+1 (B was issued one K-step ago)
        __syncthreads();
        if (it + 1 >= p.nk) break;
        issue(it + 3, xb, wb);
        compute(1);                  // tile it+1
        stash(0, xa, wa);            // tile it+2
        __syncthreads();
    }

    // the last K-step's barrier has passed: the stage buffers are idle and become the per-wave transpose slices
    epilogue_wave<T, MC, MP>(p, acc, smem + wv * (MP * 32 * MC * 64), ct * TC + wc * MC * 32, pt * TP + wp * MP * 32, lane, pt * WAVES_P + wp);
}

// ---- v3: LDS-DMA staging.  `buffer_load_dwordx4 ... lds` moves each wave's 1 KiB chunk straight from L2/HBM into
// the LDS tile (no VGPR round trip, no ds_write pass); the destination is lane-linear, so the XOR swizzle is applied
// to the SOURCE address (lane = physical slot, it fetches the logical slot that belongs there) and again on the
// fragment read.  Out-of-range lanes (halo, tails, K padding) carry offset 0xffffffff: the descriptor's bounds check
// makes them land as zeros.  Two LDS stages, ONE barrier per K-step: the barrier both publishes tile t (each wave's
// vmcnt(0) precedes it) and retires the reads of the stage tile t+1 is about to overwrite.  Fragments are
// double-buffered in registers so the ds_read of k-substep s+1 is in flight under the MFMAs of s.
// WAVES 2x2; per-wave tile (MC*32 couts) x (MP*32 pixels).
template <typename T, int BK, int MC, int MP>
Y3_DEV void conv_igemm_v3_body(const ConvArgs& p, const int block_id, const int n_blocks) {
#if defined(__HIP_DEVICE_COMPILE__)  // device-only builtins (LDS address space, buffer->LDS DMA): the host pass only needs the stub
    constexpr int WAVES_C = 2, WAVES_P = 2;
    constexpr int TC = WAVES_C * MC * 32;
    constexpr int TP = WAVES_P * MP * 32;
    constexpr int S = BK / 8;
    constexpr int WJ = TC * S / 256;
    constexpr int XJ = TP * S / 256;
    static_assert((TC * S) % 256 == 0 && (TP * S) % 256 == 0, "whole chunks only");
    constexpr int W_BYTES = TC * BK * 2;
    constexpr int STAGE_BYTES = (TC + TP) * BK * 2;
    constexpr int LDS_BYTES = 2 * STAGE_BYTES > TC * TP * 2 ? 2 * STAGE_BYTES : TC * TP * 2;  // K-loop stages, re-used as the epilogue's T-typed output tile
    constexpr int ROWSTEP = 256 / S;
    constexpr int KSUB = BK / 16;
    typedef typename Mfma<T>::frag frag;
    typedef __attribute__((address_space(3))) void* lds_ptr_t;

    __shared__ __attribute__((aligned(16))) unsigned char smem[LDS_BYTES];

    Y3_STAMP(0);
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wc = wv / WAVES_P, wp = wv % WAVES_P;

    const int L = xcd_remap(block_id, n_blocks);
    const int pt = fdiv(L, p.dv_ct_mul, p.dv_ct_sh), ct = L - pt * p.n_ct;

    const auto rsrc_x = __builtin_amdgcn_make_buffer_rsrc((void*)p.x, 0, (int)p.x_bytes, 0x00020000);
    const auto rsrc_w = __builtin_amdgcn_make_buffer_rsrc((void*)p.w, 0, (int)p.w_bytes, 0x00020000);
    constexpr unsigned OOB = 0xffffffffu;

    const int pslot = tid % S;   // physical 16-byte slot this lane fills in every row it touches
    const int row0 = tid / S;

    int xoff[XJ], hi0[XJ], wi0[XJ], xc0[XJ], xlin0[XJ];
    bool mvalid[XJ];
#pragma unroll
    for (int j = 0; j < XJ; ++j) {
        const int row = row0 + j * ROWSTEP;
        const int m = pt * TP + row;
        const bool v = m < p.M;
        const int mm = v ? m : 0;
        int n, ho, wo;
        pix_coords(mm, p, n, ho, wo);
        hi0[j] = ho * p.stride - p.pad;
        wi0[j] = wo * p.stride - p.pad;
        xoff[j] = (int)(((long long)n * p.H * p.W * p.xpitch) * 2);  // byte offset of image n
        xc0[j] = ((pslot ^ swz<BK>(row)) * 8) * 2;          // byte offset of the logical slot inside the K-step
        mvalid[j] = v;
        // plain (non-dilated) input: the lane's offset is a per-lane constant + a per-K-step SCALAR ((kh W + kw) xpitch + channel block), see dma
        xlin0[j] = xoff[j] + ((hi0[j] * p.W + wi0[j]) * p.xpitch) * 2 + xc0[j];
    }
    const bool plain_x = p.dil_shift == 0;   // kernel-uniform
    unsigned woff[WJ];
#pragma unroll
    for (int j = 0; j < WJ; ++j) {
        const int row = row0 + j * ROWSTEP;
        woff[j] = (unsigned)(((long long)(ct * TC + row) * p.Kpad + (pslot ^ swz<BK>(row)) * 8) * 2);
    }

    int nx_tap = 0, nx_cb = 0, nx_kh, nx_kw;   // (tap, channel block) of the next tile to be requested: K-steps are issued strictly in order
    tap_offsets(p, 0, nx_kh, nx_kw);
    auto dma = [&](int it, int stage) {
        const int cb = nx_cb, kh = nx_kh, kw = nx_kw;
        if (++nx_cb == p.cin_blocks) { nx_cb = 0; ++nx_tap; tap_offsets(p, nx_tap, nx_kh, nx_kw); }
        unsigned char* wl = smem + stage * STAGE_BYTES;
        unsigned char* xl = wl + W_BYTES;
#pragma unroll
        for (int j = 0; j < WJ; ++j)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_w, (lds_ptr_t)(wl + (j * 256 + wv * 64) * 16), 16, woff[j] + (unsigned)(it * BK * 2), 0, 0, 0);
        if (plain_x) {
            // (round 3) no multiplication per piece: the per-K-step part of the offset is scalar
            const int s_tap = ((kh * p.W + kw) * p.xpitch + cb * BK) * 2;
#pragma unroll
            for (int j = 0; j < XJ; ++j) {
                const int hi = hi0[j] + kh, wi = wi0[j] + kw;
                const bool ok = (int)mvalid[j] & (int)((unsigned)hi < (unsigned)p.H) & (int)((unsigned)wi < (unsigned)p.W);
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_x, (lds_ptr_t)(xl + (j * 256 + wv * 64) * 16), 16, ok ? (unsigned)(xlin0[j] + s_tap) : OOB, 0, 0, 0);
            }
        } else {
#pragma unroll
            for (int j = 0; j < XJ; ++j) {
                const int hi = hi0[j] + kh, wi = wi0[j] + kw;
                const bool ok = (int)mvalid[j] & (int)in_image(hi, wi, p);
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_x, (lds_ptr_t)(xl + (j * 256 + wv * 64) * 16), 16,
                                                         ok ? (unsigned)(xoff[j] + tap_bytes(hi0[j], wi0[j], kh, kw, cb * BK, p) + xc0[j]) : OOB, 0, 0, 0);
            }
        }
    };

    const int frow = lane & 31;
    const int fk = lane >> 5;

    // the accumulators start at the bias of their filter (lane holds filters 8g + 4fk + q of each 32-filter tile): the
    // loads overlap the first tile's flight and the epilogue has no bias pass
    f32x16 acc[MC][MP];
#pragma unroll
    for (int a = 0; a < MC; ++a)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int cb = ct * TC + (wc * MC + a) * 32 + 8 * g + 4 * fk;
            f32x4 bz = {0.f, 0.f, 0.f, 0.f};
            if (p.bias && cb + 4 <= p.Cout) bz = *(const f32x4*)(p.bias + cb);
#pragma unroll
            for (int b = 0; b < MP; ++b)
#pragma unroll
                for (int q = 0; q < 4; ++q) acc[a][b][4 * g + q] = bz[q];
        }

    auto load_frags = [&](int stage, int kk, frag (&af)[MC], frag (&bf)[MP]) {
        const unsigned char* wl = smem + stage * STAGE_BYTES;
        const unsigned char* xl = wl + W_BYTES;
        const int ks = kk * 2 + fk;
#pragma unroll
        for (int a = 0; a < MC; ++a) {
            const int row = (wc * MC + a) * 32 + frow;
            af[a] = *(const frag*)(wl + row * (BK * 2) + ((ks ^ swz<BK>(row)) << 4));
        }
#pragma unroll
        for (int b = 0; b < MP; ++b) {
            const int row = (wp * MP + b) * 32 + frow;
            bf[b] = *(const frag*)(xl + row * (BK * 2) + ((ks ^ swz<BK>(row)) << 4));
        }
    };
    auto mma = [&](const frag (&af)[MC], const frag (&bf)[MP]) {
#pragma unroll
        for (int a = 0; a < MC; ++a)
#pragma unroll
            for (int b = 0; b < MP; ++b) acc[a][b] = Mfma<T>::run(af[a], bf[b], acc[a][b]);
    };

    dma(0, 0);
    Y3_STAMP(1);
    for (int it = 0; it < p.nk; ++it) {
        __syncthreads();  // tile `it` has landed for every wave; stage (it+1)&1 is no longer being read
        if (it == 0) Y3_STAMP(2);
        if (it + 1 < p.nk) dma(it + 1, (it + 1) & 1);
        const int st = it & 1;
        frag a0[MC], b0[MP], a1[MC], b1[MP];
        load_frags(st, 0, a0, b0);
#pragma unroll
        for (int kk = 0; kk < KSUB; kk += 2) {
            load_frags(st, kk + 1, a1, b1);
            mma(a0, b0);
            if (kk + 2 < KSUB) load_frags(st, kk + 2, a0, b0);
            mma(a1, b1);
        }
    }
    Y3_STAMP(3);

    __syncthreads();  // every wave is done with the stage buffers: they become the per-wave transpose slices
    epilogue_wave<T, MC, MP>(p, acc, smem + wv * (MP * 32 * MC * 64), ct * TC + wc * MC * 32, pt * TP + wp * MP * 32, lane, pt * WAVES_P + wp);
    Y3_STAMP(4);
#endif
}

template <typename T, int BK, int MC, int MP>
__global__ __launch_bounds__(256, (BK == 32 && MC * MP <= 4 ? 4 : 2)) void conv_igemm_v3_kernel(const ConvArgs p) {
    conv_igemm_v3_body<T, BK, MC, MP>(p, blockIdx.x, gridDim.x);
}

// Four convolutions of the SAME input in one launch: the output-parity classes of a stride-2 data gradient (y3_conv2d_dgrad_s2).  As
// four launches every class streamed du from HBM again (4 x the 64-channel 320x320 map of layer 1 at batch 64 = 3.4 GB for 1.7 GB of
// output).  Block ids are laid out so that the four classes of one pixel tile are dispatched back to back on the SAME XCD
// (id = 32 * (t / 8) + 8 * class + t % 8: the XCD is id % 8 = t % 8), so three of the four reads of a du tile hit that XCD's L2.
struct ConvArgs4 {
    ConvArgs a[4];
};
template <typename T, int BK, int MC, int MP>
__global__ __launch_bounds__(256, (BK == 32 && MC * MP <= 4 ? 4 : 2)) void conv_igemm_v3_quad_kernel(const ConvArgs4 q, const int n_blocks) {
    const int cls = (blockIdx.x >> 3) & 3;
    const int bid = (int)((blockIdx.x >> 5) << 3) | (int)(blockIdx.x & 7);
    if (bid >= n_blocks) return;
    conv_igemm_v3_body<T, BK, MC, MP>(q.a[cls], bid, n_blocks);
}

// ---- v6: 8 waves (512 threads), 256 couts x 256 pixels, BK 32, the v3 staging generalised to a 4-stage LDS ring.
// Probe runs (profiles/r01_conv_probe.md) showed v3 spending as many issue cycles on `buffer_load ... lds` pieces as on the
// MFMAs they feed and its MFMA + ds_read half topping out at ~45 %: a 256x256 tile halves the staged bytes (DMA pieces)
// per MFMA and a 64c x 128p wave tile needs 0.75 fragment reads per MFMA instead of 1.  One block (8 waves) per CU.
//
// Schedule: the two halves of the block (waves 0-3 / 4-7 = one wave of each half on every SIMD) run ONE barrier interval
// apart, so while one half multiplies the other half requests tiles and reads fragments -- the MFMA pipe of a SIMD always
// has the other wave's memory phase to hide.  Per K-tile a wave does MEM(t) = { request tile t + AHEAD (4 DMA pieces),
// read the 12 fragments of tile t, counted s_waitcnt vmcnt } | barrier | MMA(t) = { 16 MFMAs } | barrier.  A tile is first read
// (by the leading half) in the interval after every wave's counted vmcnt retired its pieces of that tile and passed a barrier:
// the wait sits at the end of MEM(t-1), the reads in MEM(t).  Waits never drain to 0 in the steady state.
//   AHEAD 2 (round 1 / 2): tile t+2 lands in the stage of tile t-2, whose last reads retired two intervals ago.
//   AHEAD 3 (round 3): tile t+3 lands in the stage of tile t-1.  The probe of round 2 (profiles/r02_v7_probe.txt) had every wave
//     parked ~185 of ~1620 ticks per K-step in the counted wait -- a piece that misses L2 takes longer than the one K-step AHEAD 2
//     gives it, and vmcnt retires in order.  The last readers of stage (t-1)&3 are the trailing half's MEM(t-1), one interval
//     before the leading half's MEM(t): every wave therefore completes its fragment reads (lgkmcnt(0)) BEFORE the barrier that
//     ends its MEM phase, so that no read can still be in flight when the other half's request is issued behind that barrier.
template <int N> Y3_DEV void wait_vmcnt() {   // `s_waitcnt vmcnt(N)`; the immediate must be a literal
    static_assert(N >= 0 && N <= 12, "extend the table");
    if constexpr (N == 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    else if constexpr (N == 1) asm volatile("s_waitcnt vmcnt(1)" ::: "memory");
    else if constexpr (N == 2) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
    else if constexpr (N == 3) asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
    else if constexpr (N == 4) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    else if constexpr (N == 5) asm volatile("s_waitcnt vmcnt(5)" ::: "memory");
    else if constexpr (N == 6) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
    else if constexpr (N == 7) asm volatile("s_waitcnt vmcnt(7)" ::: "memory");
    else if constexpr (N == 8) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    else if constexpr (N == 9) asm volatile("s_waitcnt vmcnt(9)" ::: "memory");
    else if constexpr (N == 10) asm volatile("s_waitcnt vmcnt(10)" ::: "memory");
    else if constexpr (N == 11) asm volatile("s_waitcnt vmcnt(11)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(12)" ::: "memory");
}

template <typename T, int AHEAD>
__global__ __launch_bounds__(512, 2) void conv_igemm_v6_kernel(const ConvArgs p) {
#if defined(__HIP_DEVICE_COMPILE__)  // device-only builtins (LDS address space, buffer->LDS DMA): the host pass only needs the stub
    constexpr int BK = 32, WAVES_C = 4, WAVES_P = 2, MC = 2, MP = 4;
    constexpr int NT = 64 * WAVES_C * WAVES_P;
    constexpr int TC = WAVES_C * MC * 32;
    constexpr int TP = WAVES_P * MP * 32;
    constexpr int S = BK / 8;
    constexpr int WJ = TC * S / NT;
    constexpr int XJ = TP * S / NT;
    static_assert(WJ + XJ == 4 && (AHEAD == 2 || AHEAD == 3), "4 DMA pieces per wave and tile; 4 stages hold AHEAD <= 3");
    constexpr int W_BYTES = TC * BK * 2;
    constexpr int STAGE_BYTES = (TC + TP) * BK * 2;
    constexpr int NST = 4;
    constexpr int LDS_BYTES = NST * STAGE_BYTES > TC * TP * 2 ? NST * STAGE_BYTES : TC * TP * 2;  // K-loop stages, re-used as the epilogue's T-typed output tile
    constexpr int ROWSTEP = NT / S;
    typedef typename Mfma<T>::frag frag;
    typedef __attribute__((address_space(3))) void* lds_ptr_t;

    __shared__ __attribute__((aligned(16))) unsigned char smem[LDS_BYTES];

    Y3_STAMP(0);
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wc = wv / WAVES_P, wp = wv % WAVES_P;

    const int L = xcd_remap(blockIdx.x, gridDim.x);
    const int pt = fdiv(L, p.dv_ct_mul, p.dv_ct_sh), ct = L - pt * p.n_ct;

    const auto rsrc_x = __builtin_amdgcn_make_buffer_rsrc((void*)p.x, 0, (int)p.x_bytes, 0x00020000);
    const auto rsrc_w = __builtin_amdgcn_make_buffer_rsrc((void*)p.w, 0, (int)p.w_bytes, 0x00020000);
    constexpr unsigned OOB = 0xffffffffu;

    const int pslot = tid % S;   // physical 16-byte slot this lane fills in every row it touches
    const int row0 = tid / S;

    int xoff[XJ], hi0[XJ], wi0[XJ], xc0[XJ], xlin0[XJ];
    bool mvalid[XJ];
#pragma unroll
    for (int j = 0; j < XJ; ++j) {
        const int row = row0 + j * ROWSTEP;
        const int m = pt * TP + row;
        const bool v = m < p.M;
        const int mm = v ? m : 0;
        int n, ho, wo;
        pix_coords(mm, p, n, ho, wo);
        hi0[j] = ho * p.stride - p.pad;
        wi0[j] = wo * p.stride - p.pad;
        xoff[j] = (int)(((long long)n * p.H * p.W * p.xpitch) * 2);  // byte offset of image n
        xc0[j] = ((pslot ^ swz<BK>(row)) * 8) * 2;          // byte offset of the logical slot inside the K-step
        mvalid[j] = v;
        // plain (non-dilated) input: the lane's offset is a per-lane constant + a per-K-step SCALAR ((kh W + kw) xpitch + channel block), see dma
        xlin0[j] = xoff[j] + ((hi0[j] * p.W + wi0[j]) * p.xpitch) * 2 + xc0[j];
    }
    const bool plain_x = p.dil_shift == 0;   // kernel-uniform
    unsigned woff[WJ];
#pragma unroll
    for (int j = 0; j < WJ; ++j) {
        const int row = row0 + j * ROWSTEP;
        woff[j] = (unsigned)(((long long)(ct * TC + row) * p.Kpad + (pslot ^ swz<BK>(row)) * 8) * 2);
    }

    int nx_tap = 0, nx_cb = 0, nx_kh, nx_kw;   // (tap, channel block) of the next tile to be requested: K-steps are issued strictly in order
    tap_offsets(p, 0, nx_kh, nx_kw);
    auto dma = [&](int it, int stage) {
        const int cb = nx_cb, kh = nx_kh, kw = nx_kw;
        if (++nx_cb == p.cin_blocks) { nx_cb = 0; ++nx_tap; tap_offsets(p, nx_tap, nx_kh, nx_kw); }
        unsigned char* wl = smem + stage * STAGE_BYTES;
        unsigned char* xl = wl + W_BYTES;
#pragma unroll
        for (int j = 0; j < WJ; ++j)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_w, (lds_ptr_t)(wl + (j * NT + wv * 64) * 16), 16, woff[j] + (unsigned)(it * BK * 2), 0, 0, 0);
        if (plain_x) {
            const int s_tap = ((kh * p.W + kw) * p.xpitch + cb * BK) * 2;   // (round 3) the per-K-step part of the offset is scalar: no multiplication per piece
#pragma unroll
            for (int j = 0; j < XJ; ++j) {
                const int hi = hi0[j] + kh, wi = wi0[j] + kw;
                const bool ok = (int)mvalid[j] & (int)((unsigned)hi < (unsigned)p.H) & (int)((unsigned)wi < (unsigned)p.W);
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_x, (lds_ptr_t)(xl + (j * NT + wv * 64) * 16), 16, ok ? (unsigned)(xlin0[j] + s_tap) : OOB, 0, 0, 0);
            }
        } else {
#pragma unroll
            for (int j = 0; j < XJ; ++j) {
                const int hi = hi0[j] + kh, wi = wi0[j] + kw;
                const bool ok = (int)mvalid[j] & (int)in_image(hi, wi, p);
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_x, (lds_ptr_t)(xl + (j * NT + wv * 64) * 16), 16,
                                                         ok ? (unsigned)(xoff[j] + tap_bytes(hi0[j], wi0[j], kh, kw, cb * BK, p) + xc0[j]) : OOB, 0, 0, 0);
            }
        }
    };

    const int frow = lane & 31;
    const int fk = lane >> 5;

    // the accumulators start at the bias of their filter (lane holds filters 8g + 4fk + q of each 32-filter tile): the
    // loads overlap the first tile's flight and the epilogue has no bias pass
    f32x16 acc[MC][MP];
#pragma unroll
    for (int a = 0; a < MC; ++a)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int cb = ct * TC + (wc * MC + a) * 32 + 8 * g + 4 * fk;
            f32x4 bz = {0.f, 0.f, 0.f, 0.f};
            if (p.bias && cb + 4 <= p.Cout) bz = *(const f32x4*)(p.bias + cb);
#pragma unroll
            for (int b = 0; b < MP; ++b)
#pragma unroll
                for (int q = 0; q < 4; ++q) acc[a][b][4 * g + q] = bz[q];
        }

    auto load_frags = [&](int stage, int kk, frag (&af)[MC], frag (&bf)[MP]) {
        const unsigned char* wl = smem + stage * STAGE_BYTES;
        const unsigned char* xl = wl + W_BYTES;
        const int ks = kk * 2 + fk;
#pragma unroll
        for (int a = 0; a < MC; ++a) {
            const int row = (wc * MC + a) * 32 + frow;
            af[a] = *(const frag*)(wl + row * (BK * 2) + ((ks ^ swz<BK>(row)) << 4));
        }
#pragma unroll
        for (int b = 0; b < MP; ++b) {
            const int row = (wp * MP + b) * 32 + frow;
            bf[b] = *(const frag*)(xl + row * (BK * 2) + ((ks ^ swz<BK>(row)) << 4));
        }
    };
    auto mma = [&](const frag (&af)[MC], const frag (&bf)[MP]) {
#pragma unroll
        for (int a = 0; a < MC; ++a)
#pragma unroll
            for (int b = 0; b < MP; ++b) acc[a][b] = Mfma<T>::run(af[a], bf[b], acc[a][b]);
    };
    // leave the pieces of `tiles` younger K-tiles (4 per wave and tile) in flight
    auto wait_tiles = [&](int tiles) {
        if (tiles >= 2) wait_vmcnt<8>();
        else if (tiles == 1) wait_vmcnt<4>();
        else wait_vmcnt<0>();
    };

    const int half = wv >> 2;   // 0: leading half, 1: trailing half (one barrier interval behind)
    const int nk = p.nk;
    dma(0, 0);
    if (nk > 1) dma(1, 1);
    if (AHEAD == 3 && nk > 2) dma(2, 2);
    Y3_STAMP(1);
    wait_tiles(min(nk, AHEAD) - 1);
    __builtin_amdgcn_s_barrier();          // tile 0 is visible to everyone
    Y3_STAMP(2);
    if (half) __builtin_amdgcn_s_barrier();   // stagger
    for (int it = 0; it < nk; ++it) {
        // ---- MEM(it): request tile it + AHEAD, read the fragments of tile it, retire this wave's pieces of tile it + 1 ----
        if (it + AHEAD < nk) dma(it + AHEAD, (it + AHEAD) & 3);
        frag a0[MC], b0[MP], a1[MC], b1[MP];
        load_frags(it & 3, 0, a0, b0);
        load_frags(it & 3, 1, a1, b1);
        wait_tiles(min(nk - 1, it + AHEAD) - min(nk - 1, it + 1));
        if constexpr (AHEAD == 3) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // the stage just read is requested into by the other half right behind the barrier
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_barrier();
        // ---- MMA(it) ----
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_setprio(1);
        mma(a0, b0);
        mma(a1, b1);
        __builtin_amdgcn_s_setprio(0);
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_barrier();
    }
    if (!half) __builtin_amdgcn_s_barrier();  // re-align: every wave has now passed 2 nk + 2 barriers and retired all its fragment reads
    Y3_STAMP(3);
    epilogue_wave<T, MC, MP>(p, acc, smem + wv * (MP * 32 * MC * 64), ct * TC + wc * MC * 32, pt * TP + wp * MP * 32, lane, pt * WAVES_P + wp);
    Y3_STAMP(4);
#endif
}

// The launch helpers (this file, conv_v10.h, conv_strip.h, conv_1x1s.h) run on a ConvArgs whose n_ct / n_pt / stat_wp conv_launch has copied from the plan: they fill
// the rest of the kernel-visible geometry and launch.  None of them plans.
static void tile_fill(ConvArgs& a, int bk) {   // the uniform-tap tile kernels (v6, v3, v2 with Cin % BK == 0)
    set_divisors(a);
    a.cin_blocks = a.Cin / bk;
    a.nk = a.ntaps * a.cin_blocks;
}
template <typename T> int launch_v6(ConvArgs& a, hipStream_t st) {
    tile_fill(a, 32);
    const dim3 grid((unsigned)(a.n_ct * a.n_pt));
    if (y3_knob(Y3K_CONV_AHEAD) == 2) hipLaunchKernelGGL((conv_igemm_v6_kernel<T, 2>), grid, dim3(512), 0, st, a);
    else hipLaunchKernelGGL((conv_igemm_v6_kernel<T, 3>), grid, dim3(512), 0, st, a);
    Y3_CHECK_LAUNCH();
    return 0;
}
// `quad`: the four parity classes of a stride-2 data gradient (same Cout, M and channel counts; only the filter bank, the tap table and the output parity differ) go
// out as ONE launch on the tile grid of `a`, the class with the most taps
template <typename T, int BK, int MC, int MP> int launch_v3(ConvArgs& a, const ConvArgs* quad, hipStream_t st) {
    if (quad) {
        ConvArgs4 q;
        for (int i = 0; i < 4; ++i) {
            q.a[i] = quad[i];
            q.a[i].n_ct = a.n_ct; q.a[i].n_pt = a.n_pt; q.a[i].stat_wp = a.stat_wp;
            tile_fill(q.a[i], BK);
        }
        const long long nb = (long long)a.n_ct * a.n_pt;
        hipLaunchKernelGGL((conv_igemm_v3_quad_kernel<T, BK, MC, MP>), dim3((unsigned)((nb + 7) / 8 * 32)), dim3(256), 0, st, q, (int)nb);
        Y3_CHECK_LAUNCH();
        return 0;
    }
    tile_fill(a, BK);
    hipLaunchKernelGGL((conv_igemm_v3_kernel<T, BK, MC, MP>), dim3((unsigned)(a.n_ct * a.n_pt)), dim3(256), 0, st, a);
    Y3_CHECK_LAUNCH();
    return 0;
}

// ---- direct (one thread per output element) kernel: fp32 dtype path and debug cross-check -----------
template <typename T>
__global__ __launch_bounds__(256) void conv_direct_kernel(const ConvArgs p) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long total = (long long)p.M * p.Cout;
    if (idx >= total) return;
    const int c = (int)(idx % p.Cout);
    const int m = (int)(idx / p.Cout);
    const int n = m / (p.Ho * p.Wo);
    const int rem = m - n * (p.Ho * p.Wo);
    const int ho = rem / p.Wo, wo = rem - ho * p.Wo;
    const T* xg = (const T*)p.x;
    const T* wg = (const T*)p.w + (long long)c * p.Kpad;
    float acc = 0.0f;
    for (int kh = 0; kh < p.ks; ++kh) {
        const int hv = ho * p.stride - p.pad + kh;
        for (int kw = 0; kw < p.ks; ++kw) {
            const int wv = wo * p.stride - p.pad + kw;
            if (!in_image(hv, wv, p)) continue;
            const int hi = hv >> p.dil_shift, wi = wv >> p.dil_shift;
            const T* xp = xg + ((long long)(n * p.H + hi) * p.W + wi) * p.xpitch;
            const T* wp = wg + (kh * p.ks + kw) * p.Cin;
            for (int ci = 0; ci < p.Cin; ++ci) acc = fmaf(to_f32<T>(xp[ci]), to_f32<T>(wp[ci]), acc);
        }
    }
    float t = acc + p.bias[c];
    if (p.act == Y3_ACT_SILU) t = t / (1.0f + expf(-t));
    if (p.res) t += to_f32<T>(((const T*)p.res)[out_pix(n, ho, wo, p) * p.rpitch + c]);
    T* yg = (T*)p.y;
    const T o = from_f32<T>(t);
    if (!p.ups) {
        yg[out_pix(n, ho, wo, p) * p.ypitch + c] = o;
    } else {
        const int H2 = p.Ho * 2, W2 = p.Wo * 2;
        for (int dy = 0; dy < 2; ++dy)
            for (int dx = 0; dx < 2; ++dx) yg[((long long)(n * H2 + 2 * ho + dy) * W2 + 2 * wo + dx) * p.ypitch + c] = o;
    }
}

template <typename T, int BK, int WAVES_C, int WAVES_P, int MC, int MP, bool SMALLC>
int launch_igemm(ConvArgs& a, hipStream_t st) {
    tile_fill(a, BK);
    if (SMALLC) {
        a.nk = y3_ceil_div(a.ntaps * a.Cin, BK);
        a.cin_blocks = 1;
    }
    hipLaunchKernelGGL((conv_igemm_v2_kernel<T, BK, WAVES_C, WAVES_P, MC, MP, SMALLC>), dim3((unsigned)(a.n_ct * a.n_pt)), dim3(256), 0, st, a);
    Y3_CHECK_LAUNCH();
    return 0;
}

template <int I> struct IC {
    static constexpr int value = I;
};
template <typename F, int... Is> Y3_DEV void static_for_impl(F&& f, std::integer_sequence<int, Is...>) { (f(IC<Is>{}), ...); }
template <int N, typename F> Y3_DEV void static_for(F&& f) { static_for_impl(f, std::make_integer_sequence<int, N>{}); }

#include "conv_v10.h"
#include "conv_strip.h"
#include "conv_1x1s.h"

// ---- the dispatch: ONE decision (conv_decide), read by the queries and the launch ----
// The question is the filled ConvArgs of one image range (geometry and tap table, byte extents, presence of bias / residual / workspace, the input transform); the
// answer is a ConvPlan.  conv_decide is pure: it reads the arguments, the knobs and y3_cu_count() and writes nothing but the plan.
enum ConvForm { CF_DIRECT, CF_V2, CF_V3_BK64, CF_V3_128X128, CF_V3_128X256, CF_V3_64X256, CF_V6, CF_V10, CF_V10K, CF_STRIP, CF_S1 };
struct V3Tile { const char* name; int tc, tp; };   // filters x pixels of the block tile, by form - CF_V3_BK64
constexpr V3Tile V3_TILES[4] = {{"v3_bk64_128x128", 128, 128}, {"v3_bk32_128x128", 128, 128}, {"v3_bk32_128x256", 128, 256}, {"v3_bk32_64x256", 64, 256}};
struct V2Tile { int wc, wp, mc, mp; };   // waves and 32-wide MFMA tiles per wave along filters / pixels: > 64, > 32 and <= 32 filters
constexpr V2Tile V2_TILES[3] = {{2, 2, 2, 2}, {1, 4, 2, 1}, {1, 4, 1, 2}};
struct ConvPlan {
    ConvForm form;             // (the four v3 tiles are four forms)
    const char* name;          // what y3_conv2d_fwd_variant and y3_conv_last_variant report
    int tile;                  // CF_V2: 3 * (index into V2_TILES) + (0: BK 64, 1: BK 32, 2: BK 32 with Cin % 32 != 0)
    int n_pt, n_ct, stat_wp;   // the launch writes n_pt * stat_wp statistics rows
    CsPlan cs;                 // the form's own plan: CF_STRIP, CF_S1, CF_V10 / CF_V10K
    S1Plan s1;
    V10Plan v10;
    int64_t rows() const { return (int64_t)n_pt * stat_wp; }
    bool is_v3() const { return form >= CF_V3_BK64 && form <= CF_V3_64X256; }
};

static int plan_set(ConvPlan& p, ConvForm form, const char* name, int n_ct, int n_pt, int stat_wp, int tile = 0) {
    p.form = form; p.name = name; p.tile = tile;
    p.n_ct = n_ct; p.n_pt = n_pt; p.stat_wp = stat_wp;
    return 0;
}
static int plan_tile(const ConvArgs& a, ConvPlan& p, ConvForm form, const char* name, int tc, int tp, int stat_wp, int tile = 0) {   // tc filters x tp pixels per block
    if ((long long)y3_ceil_div(a.Cout, tc) * y3_ceil_div(a.M, tp) > 0x7fffffffLL) Y3_FAIL("conv grid too large");
    return plan_set(p, form, name, y3_ceil_div(a.Cout, tc), y3_ceil_div(a.M, tp), stat_wp, tile);
}
static int s1_in(const ConvArgs& a) { return a.in_scale ? (a.in_res ? 2 : 1) : 0; }
// the s1 form of a plan whose p.s1 is filled: stages along the pixels, one statistics row per (pixel wave, epilogue pass) of a stage
static int plan_s1(const ConvArgs& a, ConvPlan& p) { return plan_set(p, CF_S1, p.s1.in ? "s1x1_bn" : "s1x1", p.s1.n_ct, y3_ceil_div(a.M, p.s1.sp), p.s1.wp * p.s1.npass); }

static int conv_decide(const ConvArgs& a, ConvPlan& p, bool direct = false) {
    if (direct) return plan_set(p, CF_DIRECT, "direct", 0, 0, 0);   // fp32 / Y3_ALGO_DIRECT: one thread per output element
    const bool c64 = (a.Cin % 64) == 0, c32 = (a.Cin % 32) == 0;
    const int var = conv_variant();
    auto v3 = [&](ConvForm f) { return plan_tile(a, p, f, V3_TILES[f - CF_V3_BK64].name, V3_TILES[f - CF_V3_BK64].tc, V3_TILES[f - CF_V3_BK64].tp, 2); };
    auto v6 = [&]() { return plan_tile(a, p, CF_V6, "v6", 256, 256, 2); };
    if (!(a.x_bytes && a.w_bytes && a.y_bytes && (!a.res || a.r_bytes)))
        Y3_FAIL("conv: a tensor exceeds the 2 GiB reach of a buffer descriptor (split the batch)");
    if (var == 3 && cs_plan(a, p.cs)) return plan_set(p, CF_STRIP, "strip", 1, p.cs.blocks, p.cs.mt * (a.Cin > 64 ? 2 : 1));   // one statistics row per block, pixel tile and K-split wave
    if (var == 3 && s1_plan(a, p.s1, s1_in(a))) return plan_s1(a, p);   // HBM-bound 1x1 layers: persistent blocks, filters in registers (conv_1x1s.h)
    if (var == 3 && v10_shape_ok(a)) {
        // conv_v10.h: a quarter round of tiles or more takes the tile form (statistics rows per tile: one per 64-pixel epilogue pass of the widest body, narrower bodies
        // write zero rows), smaller launches with a workspace the K-split form (one row per 64-pixel block of the slab sum); knob v10_ksplit = 2: the K-split form on
        // any eligible launch (tests)
        const long long ksplit = y3_knob(Y3K_V10_KSPLIT);
        const bool big = v10_big_enough(a);
        if (ksplit == 2 && v10k_plan(a, p.v10)) return plan_set(p, CF_V10K, "v10k", a.Cout / 256, y3_ceil_div(a.M, 64), 1);
        if (big && v10_plan(a, p.v10)) return plan_set(p, CF_V10, p.v10.half ? "v10h" : "v10", a.Cout / 256, p.v10.n_tiles, 4);
        if (ksplit != 0 && ksplit != 2 && !big && v10k_plan(a, p.v10)) return plan_set(p, CF_V10K, "v10k", a.Cout / 256, y3_ceil_div(a.M, 64), 1);
    }
    if (var >= 3 && a.Cout > 64 && c32) {
        // forced tiles (knob "conv", A/B runs)
        if (var == 4) return v3(CF_V3_128X256);   // 128c x 256p, BK 32
        if (var == 5) return v3(CF_V3_128X128);   // 128c x 128p, BK 32 (4 blocks / CU)
        if (var == 6) return v3(c64 ? CF_V3_BK64 : CF_V3_128X128);
        if (var == 15 && a.Cout >= 256) return v6();
        // auto (measured on MI355X, profiles/r01_conv_variants.md, r02_conv_variant_sweep.txt): long-K layers with >= 512 filters want
        // the 8-wave 256x256 tile (v6), short K loops want 4 resident blocks per CU (BK 32), small pixel counts with long K the
        // 128x256 tile, the rest the BK 64 128x128 tile.
        const int K = a.ntaps * a.Cin;
        if (K >= 2304 && a.Cout >= 512) return v6();
        if (K >= 4608 && a.Cout >= 256 && a.M >= 65536) return v6();   // data gradient of the 256 -> 512 layers (one filter tile)
        if (c64 && a.ntaps == 1 && a.Cout >= 256 && a.M > 16384 && a.M <= 65536) return v6();   // 1x1 @40x40
        if (c64 && ((a.ntaps > 1 && K >= 1152) || (a.ntaps == 1 && K >= 256 && a.M <= 16384))) return v3(CF_V3_BK64);
        // 64 -> 128 3x3 @160x160 runs 5 % faster on the 128c x 256p tile, the stride-2 64 -> 128 layer 3 % faster with BK 64
        if (c64 && a.ntaps > 1 && K == 576 && a.Cout == 128 && a.M >= 262144) return v3(a.stride == 1 ? CF_V3_128X256 : CF_V3_BK64);
        return v3(CF_V3_128X128);
    }
    // <= 64-filter layers with Cin % 32 == 0 also go to the LDS-DMA kernel (64c x 256p tile): measured 0.42 -> 0.36 ms on
    // 32->64 s2 @640x640 and 0.44 -> 0.38 ms on 32->64 @320x320 (bs 32)
    if (var != 2 && a.Cout <= 64 && c32) return v3(CF_V3_64X256);   // 64c x 256p, wave 32c x 128p
    // register-staged fallback: Cin % 32 != 0 (layer 0 when the stem kernel is not eligible)
    const int fc = a.Cout > 64 ? 0 : (a.Cout > 32 ? 1 : 2), kc = c64 ? 0 : (c32 ? 1 : 2);
    const V2Tile& t = V2_TILES[fc];
    return plan_tile(a, p, CF_V2, kc == 2 ? "v2_smallc" : "v2", t.wc * t.mc * 32, t.wp * t.mp * 32, t.wp, 3 * fc + kc);
}

template <typename T> int launch_direct(ConvArgs& a, hipStream_t st) {
    const long long total = (long long)a.M * a.Cout;
    hipLaunchKernelGGL((conv_direct_kernel<T>), dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, a);
    Y3_CHECK_LAUNCH();
    return 0;
}
template <typename T, int F, int BK, bool SMALLC> int launch_v2(ConvArgs& a, hipStream_t st) {
    return launch_igemm<T, BK, V2_TILES[F].wc, V2_TILES[F].wp, V2_TILES[F].mc, V2_TILES[F].mp, SMALLC>(a, st);
}

// the launch of a decided plan (f16 / bf16; the direct form: conv_launch_as): a switch into one helper per form.  Never plans.
template <typename T> int conv_launch(ConvArgs& a, const ConvPlan& p, hipStream_t st, const ConvArgs* quad = nullptr) {
    switch (p.form) {
        case CF_STRIP: return launch_cs<T>(a, p.cs, st);
        case CF_S1: return launch_s1<T>(a, p.s1, st);
        case CF_V10K: return launch_v10k<T>(a, p.v10, st);
        case CF_V10: return launch_v10<T>(a, p.v10, st);
        case CF_V3_128X256: return launch_v3<T, 32, 2, 4>(a, quad, st);
        case CF_V3_128X128: return launch_v3<T, 32, 2, 2>(a, quad, st);
        case CF_V3_BK64: return launch_v3<T, 64, 2, 2>(a, quad, st);
        case CF_V6: return launch_v6<T>(a, st);
        case CF_V3_64X256: return launch_v3<T, 32, 1, 4>(a, quad, st);
        case CF_V2:
            switch (p.tile) {
                case 0: return launch_v2<T, 0, 64, false>(a, st);
                case 1: return launch_v2<T, 0, 32, false>(a, st);
                case 2: return launch_v2<T, 0, 32, true>(a, st);
                case 3: return launch_v2<T, 1, 64, false>(a, st);
                case 4: return launch_v2<T, 1, 32, false>(a, st);
                case 5: return launch_v2<T, 1, 32, true>(a, st);
                case 6: return launch_v2<T, 2, 64, false>(a, st);
                case 7: return launch_v2<T, 2, 32, false>(a, st);
                default: return launch_v2<T, 2, 32, true>(a, st);
            }
        default: Y3_FAIL("conv: no launch for form %d (internal)", (int)p.form);
    }
}

}  // namespace

// ---- step 1: validate the call and fill the arguments of the whole batch and the image ranges it is launched as ----
struct ConvProblem {
    ConvArgs a;                     // the whole batch
    const y3_tensor *x, *y, *res;   // (res may be null)
    int dtype, esz, chunk;          // element bytes, images per range
    bool direct;                    // fp32 / Y3_ALGO_DIRECT: the one-thread-per-element kernel
    long long opx_img, img_x, img_y, img_r, wb;   // per image: output pixels, bytes of x / y / residual; bytes of the filter bank
};
static int conv_problem(const y3_conv_desc* d, const y3_tensor* x, const void* filt, const float* bias, const y3_tensor* res, const y3_tensor* y, bool stats, void* ws,
                        size_t ws_bytes, ConvProblem& pb) {
    if (!d || !x || !filt || !bias || !y) Y3_FAIL("y3_conv2d_fwd: null argument");
    if (d->ksize != 1 && d->ksize != 3) Y3_FAIL("y3_conv2d_fwd: ksize %d unsupported", d->ksize);
    if (d->stride != 1 && d->stride != 2) Y3_FAIL("y3_conv2d_fwd: stride %d unsupported", d->stride);
    if (x->c != d->cin) Y3_FAIL("y3_conv2d_fwd: x has %d channels, filter expects %d", x->c, d->cin);
    if ((d->cin % 8) || (d->cout % 8)) Y3_FAIL("y3_conv2d_fwd: cin/cout must be multiples of 8 (%d/%d)", d->cin, d->cout);
    const int pad = d->ksize / 2;
    const int dil = d->in_dilation == 2 ? 2 : 1;
    if (d->in_dilation != 0 && d->in_dilation != 1 && d->in_dilation != 2) Y3_FAIL("y3_conv2d_fwd: in_dilation %d unsupported", d->in_dilation);
    if (dil == 2 && (d->stride != 1 || d->upsample2x)) Y3_FAIL("y3_conv2d_fwd: in_dilation 2 needs stride 1 and no upsample");
    // dilated input (stride-2 dgrad): the output size is the caller's (2h-1 or 2h, the forward conv's input size)
    int Ho = (x->h + 2 * pad - d->ksize) / d->stride + 1;
    int Wo = (x->w + 2 * pad - d->ksize) / d->stride + 1;
    if (dil == 2) {
        if (y->h != 2 * x->h && y->h != 2 * x->h - 1) Y3_FAIL("y3_conv2d_fwd: dilated output height %d does not match input %d", y->h, x->h);
        if (y->w != 2 * x->w && y->w != 2 * x->w - 1) Y3_FAIL("y3_conv2d_fwd: dilated output width %d does not match input %d", y->w, x->w);
        Ho = y->h;
        Wo = y->w;
    }
    const int up = d->upsample2x ? 2 : 1;
    if (y->n != x->n || y->h != Ho * up || y->w != Wo * up || y->c != d->cout)
        Y3_FAIL("y3_conv2d_fwd: output is (%d,%d,%d,%d), expected (%d,%d,%d,%d)", y->n, y->h, y->w, y->c, x->n, Ho * up, Wo * up, d->cout);
    if (res && (res->n != x->n || res->h != Ho || res->w != Wo || res->c != d->cout)) Y3_FAIL("y3_conv2d_fwd: residual shape mismatch");
    if (res && d->upsample2x) Y3_FAIL("y3_conv2d_fwd: residual + upsample2x unsupported");
    const int esz = d->dtype == Y3_F32 ? 4 : 2;
    const int vec = 16 / esz;
    if (d->dtype != Y3_F32) {
        if ((x->pitch % vec) || (y->pitch % vec) || (res && (res->pitch % vec)) || ((uintptr_t)x->data & 15) || ((uintptr_t)y->data & 15) ||
            (res && ((uintptr_t)res->data & 15)) || ((uintptr_t)filt & 15) || ((uintptr_t)bias & 15))   // (conv_v10.h loads the bias as f32x4)
            Y3_FAIL("y3_conv2d_fwd: tensors, filter bank and bias must be 16-byte aligned with pitch %% %d == 0", vec);
    }
    // a bank without the fragment-ordered second copy (sized rows x Kpad by the ABI-1 rule, or an old cached one) would be read past its end by conv_v10.h
    if (d->filter_elems != 0 && (uint64_t)d->filter_elems < (uint64_t)y3_packed_filter_elems(d->cout, d->cin, d->ksize))
        Y3_FAIL("y3_conv2d_fwd: the packed filter bank holds %lld elements, (cout %d, cin %d, k %d) needs %llu (size banks with y3_packed_filter_elems)",
                (long long)d->filter_elems, d->cout, d->cin, d->ksize, (unsigned long long)y3_packed_filter_elems(d->cout, d->cin, d->ksize));
    if ((long long)x->n * Ho * Wo * (d->upsample2x ? 4 : 1) > 0x7fffffffLL) Y3_FAIL("y3_conv2d_fwd: too many output pixels");

    ConvArgs& a = pb.a;
    memset(&a, 0, sizeof(a));
    a.x = x->data; a.w = filt; a.bias = bias; a.res = res ? res->data : nullptr; a.y = y->data;
    a.ws = ws; a.ws_bytes = ws ? ws_bytes : 0;
    a.N = x->n; a.H = x->h; a.W = x->w; a.Cin = d->cin; a.xpitch = x->pitch;
    a.Ho = Ho; a.Wo = Wo; a.Cout = d->cout; a.ypitch = y->pitch; a.rpitch = res ? res->pitch : 0;
    a.ks = d->ksize; a.stride = d->stride; a.pad = pad; a.act = d->act; a.ups = d->upsample2x ? 1 : 0;
    a.dil_shift = dil == 2 ? 1 : 0;
    a.ntaps = d->ksize * d->ksize;
    for (int t = 0; t < a.ntaps; ++t) { a.tdh[t] = (signed char)(t / d->ksize); a.tdw[t] = (signed char)(t % d->ksize); }
    a.oH = Ho; a.oW = Wo; a.omul = 1; a.ooh = 0; a.oow = 0;
    a.M = x->n * Ho * Wo;
    a.Kpad = y3_filter_kpad(d->cin, d->ksize);
#ifdef Y3_TIMELINE
    a.tl = g_timeline;
#endif
    int algo = d->algo;
    if (algo == Y3_ALGO_AUTO) algo = (d->dtype == Y3_F32) ? Y3_ALGO_DIRECT : Y3_ALGO_MFMA;
    if (stats) {
        if (algo != Y3_ALGO_MFMA || d->dtype == Y3_F32) Y3_FAIL("y3_conv2d_fwd_stats: the epilogue statistics need the f16/bf16 MFMA path");
        if (d->upsample2x) Y3_FAIL("y3_conv2d_fwd_stats: upsample2x unsupported");
    }

    // The MFMA kernels address every tensor through a buffer descriptor (bounds-checked loads are what makes halo / tail lanes free),
    // and a descriptor reaches 2^31 bytes.  Images are independent, so a batch whose input, output or residual exceeds that is run
    // as several launches over image ranges (batch 128 @640x640 and batch 32 @1280x1280 need it for the first layers); the
    // reference has no such limit (ATen indexes with 64 bits).
    const long long opx_img = (long long)Ho * Wo * (d->upsample2x ? 4 : 1);
    const long long img_x = (long long)x->h * x->w * x->pitch * esz, img_y = opx_img * y->pitch * esz, img_r = res ? opx_img * res->pitch * esz : 0;
    const long long LIM = 0x7fffffffLL - 65536;
    const long long wb = (long long)y3_filter_rows(d->cout) * a.Kpad * esz;
    if (wb >= LIM) Y3_FAIL("y3_conv2d_fwd: filter bank beyond 2 GiB");
    int chunk = x->n;
    if (algo == Y3_ALGO_MFMA) {
        if (img_x >= LIM || img_y >= LIM || img_r >= LIM) Y3_FAIL("y3_conv2d_fwd: one image exceeds the 2 GiB reach of a buffer descriptor");
        while (chunk > 1 && ((long long)chunk * img_x >= LIM || (long long)chunk * img_y >= LIM || (long long)chunk * img_r >= LIM))
            chunk = (chunk + 1) / 2;
    }
    pb.x = x; pb.y = y; pb.res = res;
    pb.dtype = d->dtype; pb.esz = esz; pb.chunk = chunk; pb.direct = algo != Y3_ALGO_MFMA;
    pb.opx_img = opx_img; pb.img_x = img_x; pb.img_y = img_y; pb.img_r = img_r; pb.wb = wb;
    return 0;
}
// the arguments of the image range that starts at image n0
static ConvArgs conv_range(const ConvProblem& pb, int n0) {
    const y3_tensor *x = pb.x, *y = pb.y, *res = pb.res;
    const int esz = pb.esz;
    const ConvArgs& a = pb.a;
    ConvArgs c = a;
    c.N = x->n - n0 < pb.chunk ? x->n - n0 : pb.chunk;
    c.M = c.N * a.Ho * a.Wo;
    c.x = (const char*)a.x + (long long)n0 * pb.img_x;
    c.y = (char*)a.y + (long long)n0 * pb.img_y;
    if (res) c.res = (const char*)a.res + (long long)n0 * pb.img_r;
    const long long xb = (((long long)c.N * x->h * x->w - 1) * x->pitch + x->c) * esz;
    const long long yb = (((long long)c.N * pb.opx_img - 1) * y->pitch + y->c) * esz, rb = res ? (((long long)c.N * pb.opx_img - 1) * res->pitch + res->c) * esz : 0;
    c.x_bytes = xb < 0x7fffffffLL ? (unsigned)xb : 0u;   // only the fp32 direct kernel (64-bit indexing) ever sees a 0 here
    c.w_bytes = (unsigned)pb.wb;
    c.y_bytes = yb < 0x7fffffffLL ? (unsigned)yb : 0u;
    c.r_bytes = rb < 0x7fffffffLL ? (unsigned)rb : 0u;
    return c;
}

// ---- step 3: the launch of a plan.  Every launch starts here: the plan's geometry into the kernel arguments, its name into the record behind y3_conv_last_variant
static void launch_begin(ConvArgs& a, const ConvPlan& p) {
    a.n_ct = p.n_ct; a.n_pt = p.n_pt; a.stat_wp = p.stat_wp;
    g_last_variant = p.name;
}
static int conv_launch_as(int dtype, ConvArgs& a, const ConvPlan& p, hipStream_t st) {
    launch_begin(a, p);
    if (p.form != CF_DIRECT) {
        if (dtype == Y3_F16) return conv_launch<f16_t>(a, p, st);
        if (dtype == Y3_BF16) return conv_launch<bf16_t>(a, p, st);
        Y3_FAIL("y3_conv2d_fwd: MFMA path needs f16/bf16");
    }
    switch (dtype) {
        case Y3_F16: return launch_direct<f16_t>(a, st);
        case Y3_BF16: return launch_direct<bf16_t>(a, st);
        case Y3_F32: return launch_direct<float>(a, st);
        default: Y3_FAIL("y3_conv2d_fwd: bad dtype %d", dtype);
    }
}

// validate and fill; per image range decide ONCE (step 2: a statistics launch takes its rows from that plan) and launch that plan
static int conv_fwd_impl(const y3_conv_desc* d, const y3_tensor* x, const void* filt, const float* bias, const y3_tensor* res, const y3_tensor* y, float* stats,
                         int64_t stat_capacity_rows, int64_t* stat_rows, void* stream, void* ws = nullptr, size_t ws_bytes = 0) {
    ConvProblem pb;
    if (const int rc = conv_problem(d, x, filt, bias, res, y, stat_rows != nullptr, ws, ws_bytes, pb)) return rc;
    if (stat_rows) *stat_rows = 0;
    for (int n0 = 0; n0 < pb.a.N; n0 += pb.chunk) {
        ConvArgs c = conv_range(pb, n0);
        ConvPlan p;
        if (const int rc = conv_decide(c, p, pb.direct)) return rc;
        if (stat_rows) {   // BatchNorm statistics in the epilogue
            const int64_t rows_done = *stat_rows;
            *stat_rows += p.rows();
            if (!stats || stat_capacity_rows < *stat_rows)
                Y3_FAIL("y3_conv2d_fwd_stats: statistics buffer holds %lld rows, the launch writes %lld", (long long)stat_capacity_rows, (long long)*stat_rows);
            c.stats = stats + rows_done * (int64_t)c.Cout * 2;
        }
        if (const int rc = conv_launch_as(pb.dtype, c, p, (hipStream_t)stream)) return rc;
    }
    return 0;
}

extern "C" int y3_conv2d_fwd(const y3_conv_desc* d, const y3_tensor* x, const void* filt, const float* bias, const y3_tensor* res, const y3_tensor* y, void* stream) {
    return conv_fwd_impl(d, x, filt, bias, res, y, nullptr, 0, nullptr, stream);
}

// ---- the same convolution with a scratch buffer: unlocks the K-split form of conv_v10.h for small launches ----
constexpr size_t Y3_CONV_WS_BYTES = 64 + 4 * 1024 + 2 * (size_t)256 * 256 * 256 * 4;   // 134 MB: the size round 2 fixed (callers allocate it once per plan)
extern "C" size_t y3_conv_workspace_bytes(void) { return Y3_CONV_WS_BYTES; }

extern "C" int y3_conv2d_fwd_ws(const y3_conv_desc* d, const y3_tensor* x, const void* filt, const float* bias, const y3_tensor* res, const y3_tensor* y, void* workspace,
                                size_t workspace_bytes, void* stream) {
    if (workspace && ((uintptr_t)workspace & 255)) Y3_FAIL("y3_conv2d_fwd_ws: the workspace must be 256-byte aligned");
    return conv_fwd_impl(d, x, filt, bias, res, y, nullptr, 0, nullptr, stream, workspace, workspace_bytes);
}

// ---- the queries: validate, fill and decide as the launch does, then read the plan (nothing is launched, nothing recorded) ----
alignas(256) static const float g_dummy[64] = {0.0f};   // stands for filter bank, bias, residual and workspace: never dereferenced
// the plan (and arguments) of the first image range; with `rows`, the statistics rows summed over all ranges
static int conv_query(const y3_conv_desc* d, const y3_tensor* x, const y3_tensor* y, int32_t has_residual, size_t ws_bytes, ConvArgs& c0, ConvPlan& p0, int64_t* rows) {
    y3_tensor r;
    if (has_residual && y) { r = *y; if (d && d->upsample2x) { r.h /= 2; r.w /= 2; } r.data = (void*)g_dummy; }
    ConvProblem pb;
    if (const int rc = conv_problem(d, x, (const void*)g_dummy, g_dummy, has_residual ? &r : nullptr, y, rows != nullptr, ws_bytes ? (void*)g_dummy : nullptr, ws_bytes, pb)) return rc;
    if (rows) *rows = 0;
    if (pb.a.N < 1) return plan_set(p0, CF_DIRECT, "direct", 0, 0, 0);   // an empty batch launches nothing
    c0 = conv_range(pb, 0);
    if (const int rc = conv_decide(c0, p0, pb.direct)) return rc;
    if (!rows) return 0;
    *rows = p0.rows();
    for (int n0 = pb.chunk; n0 < pb.a.N; n0 += pb.chunk) {
        ConvPlan p;
        if (const int rc = conv_decide(conv_range(pb, n0), p, pb.direct)) return rc;
        *rows += p.rows();
    }
    return 0;
}

// name of the kernel variant the dispatcher picks for this problem: "direct", "v2", "v2_smallc", "v3_bk64_128x128", "v6", "v10", "v10h", "v10k", "strip", "s1x1", ...
// (a batch launched as several image ranges: the first range's)
extern "C" int y3_conv2d_fwd_variant(const y3_conv_desc* d, const y3_tensor* x, const y3_tensor* y, int32_t has_residual, size_t workspace_bytes, char* name, size_t name_cap) {
    if (!name || name_cap < 2) Y3_FAIL("y3_conv2d_fwd_variant: no room for the name");
    ConvArgs a;
    ConvPlan p;
    if (const int rc = conv_query(d, x, y, has_residual, workspace_bytes, a, p, nullptr)) return rc;
    strncpy(name, p.name, name_cap - 1);
    name[name_cap - 1] = 0;
    return 0;
}

// The tiles of the persistent 3x3 kernel for this problem, as its blocks compute them: one record (block of the filter tile, tile of the block,
// first 32-pixel column block, column blocks) per tile of ONE filter tile, from the very functions the kernel runs (v10_share / v10_tile_cols, conv_v10.h)
extern "C" int y3_conv_v10_tiles(const y3_conv_desc* d, const y3_tensor* x, const y3_tensor* y, size_t workspace_bytes, int32_t* records, int64_t capacity, int64_t* n_tiles,
                                 int32_t* column_blocks, int32_t* group_blocks) {
    if (!n_tiles) Y3_FAIL("y3_conv_v10_tiles: null argument");
    ConvArgs a;
    ConvPlan p;
    if (const int rc = conv_query(d, x, y, 0, workspace_bytes, a, p, nullptr)) return rc;
    if (p.form != CF_V10 && p.form != CF_V10K) Y3_FAIL("y3_conv_v10_tiles: the dispatcher picks '%s' for this problem, not conv_v10.h", p.name);
    v10_fill_args(a, p.v10);
    int64_t n = 0;
    for (int bi = 0; bi < a.v10_B; ++bi) {
        const V10Share sh = v10_share(a, bi, bi / a.v10_g);
        for (int t = 0; t < sh.nt; ++t, ++n) {
            int c0, sz;
            v10_tile_cols(a, sh, t, c0, sz);
            if (records && n < capacity) { records[4 * n] = bi; records[4 * n + 1] = t; records[4 * n + 2] = c0; records[4 * n + 3] = sz; }
        }
    }
    *n_tiles = n;
    if (column_blocks) *column_blocks = (a.M + 31) / 32;
    if (group_blocks) *group_blocks = a.v10_g;
    return 0;
}

// name of the kernel variant the LAST conv / data-gradient call of this thread launched ("v3_quad" = the four parity classes of a
// stride-2 data gradient in one launch): tests assert the path they mean to exercise
extern "C" int y3_conv_last_variant(char* name, size_t name_cap) {
    if (!name || name_cap < 2) Y3_FAIL("y3_conv_last_variant: no room for the name");
    strncpy(name, g_last_variant, name_cap - 1);
    name[name_cap - 1] = 0;
    return 0;
}

// rows of the statistics buffer the launch described by (desc, x, y) would write (depends on the tile variant dispatched)
extern "C" int64_t y3_conv2d_fwd_stats_rows(const y3_conv_desc* d, const y3_tensor* x, const y3_tensor* y) { return y3_conv2d_fwd_stats_rows_ws(d, x, y, 0); }

extern "C" int y3_conv2d_fwd_stats(const y3_conv_desc* d, const y3_tensor* x, const void* filt, const float* bias, const y3_tensor* y, float* stat_rows, int64_t capacity_rows,
                                   int64_t* n_rows, void* stream) {
    if (!n_rows) Y3_FAIL("y3_conv2d_fwd_stats: null row count");
    return conv_fwd_impl(d, x, filt, bias, nullptr, y, stat_rows, capacity_rows, n_rows, stream);
}

// the two calls above with the stream-K workspace of y3_conv2d_fwd_ws (the persistent kernel writes 4 statistic rows per pixel tile)
extern "C" int64_t y3_conv2d_fwd_stats_rows_ws(const y3_conv_desc* d, const y3_tensor* x, const y3_tensor* y, size_t workspace_bytes) {
    int64_t rows = 0;
    ConvArgs a;
    ConvPlan p;
    return conv_query(d, x, y, 0, workspace_bytes, a, p, &rows) ? -1 : rows;
}

extern "C" int y3_conv2d_fwd_stats_ws(const y3_conv_desc* d, const y3_tensor* x, const void* filt, const float* bias, const y3_tensor* y, float* stat_rows,
                                      int64_t capacity_rows, int64_t* n_rows, void* workspace, size_t workspace_bytes, void* stream) {
    if (!n_rows) Y3_FAIL("y3_conv2d_fwd_stats_ws: null row count");
    if (workspace && ((uintptr_t)workspace & 255)) Y3_FAIL("y3_conv2d_fwd_stats_ws: the workspace must be 256-byte aligned");
    return conv_fwd_impl(d, x, filt, bias, nullptr, y, stat_rows, capacity_rows, n_rows, stream, workspace, workspace_bytes);
}


// ---- 1x1 convolution of act(in_scale * u + in_shift) (+ shortcut) with statistics rows: the training forward of a Bottleneck.cv1 that applies its producer's BatchNorm on the
// way in (conv_1x1s.h IN form).  `u_in` is the producer's pre-BatchNorm tensor, `y_in` receives the normalised / activated tensor (the other consumers read it), `y` this
// conv's own pre-BatchNorm output.  Shapes the form does not cover are refused (y3_conv2d_fwd_bnin_rows returns -1: the caller keeps the separate passes).
static int bnin_fill(const y3_conv_desc* d, const y3_tensor* u_in, const float* in_scale, const float* in_shift, int32_t in_act, const y3_tensor* in_res, const y3_tensor* y_in,
                     const void* filt, const float* bias, const y3_tensor* y, ConvArgs& a, ConvPlan& p) {
    if (!d || !u_in || !y_in || !y) Y3_FAIL("y3_conv2d_fwd_bnin: null argument");
    if (d->ksize != 1 || d->stride != 1 || d->upsample2x || d->in_dilation > 1 || (d->dtype != Y3_F16 && d->dtype != Y3_BF16)) Y3_FAIL("y3_conv2d_fwd_bnin: 1x1 / stride 1 / f16 or bf16 only");
    if (u_in->c != d->cin || y->c != d->cout || y_in->c != d->cin) Y3_FAIL("y3_conv2d_fwd_bnin: channel mismatch");
    if (y->n != u_in->n || y->h != u_in->h || y->w != u_in->w || y_in->n != u_in->n || y_in->h != u_in->h || y_in->w != u_in->w) Y3_FAIL("y3_conv2d_fwd_bnin: shape mismatch");
    if (in_res && (in_res->n != u_in->n || in_res->h != u_in->h || in_res->w != u_in->w || in_res->c != d->cin)) Y3_FAIL("y3_conv2d_fwd_bnin: shortcut shape mismatch");
    if ((u_in->pitch % 8) || (y->pitch % 8) || (y_in->pitch % 8) || (in_res && (in_res->pitch % 8)) || ((uintptr_t)u_in->data & 15) || ((uintptr_t)y->data & 15) ||
        ((uintptr_t)y_in->data & 15) || (in_res && ((uintptr_t)in_res->data & 15)) || ((uintptr_t)filt & 15) || ((uintptr_t)bias & 15))
        Y3_FAIL("y3_conv2d_fwd_bnin: tensors, filter bank and bias must be 16-byte aligned with pitch %% 8 == 0");
    if (d->filter_elems != 0 && (uint64_t)d->filter_elems < (uint64_t)y3_packed_filter_elems(d->cout, d->cin, 1)) Y3_FAIL("y3_conv2d_fwd_bnin: packed filter bank too short");
    const long long M = (long long)u_in->n * u_in->h * u_in->w;
    auto ext = [&](const y3_tensor* t) { return ((M - 1) * t->pitch + t->c) * 2; };
    if (M <= 0 || M > 0x7fffffffLL || ext(u_in) >= 0x7fffffffLL || ext(y) >= 0x7fffffffLL || ext(y_in) >= 0x7fffffffLL || (in_res && ext(in_res) >= 0x7fffffffLL))
        Y3_FAIL("y3_conv2d_fwd_bnin: a tensor exceeds the 2 GiB reach of a buffer descriptor");
    memset(&a, 0, sizeof(a));
    a.x = u_in->data; a.w = filt; a.bias = bias; a.y = y->data;
    a.N = u_in->n; a.H = u_in->h; a.W = u_in->w; a.Cin = d->cin; a.xpitch = u_in->pitch;
    a.Ho = a.H; a.Wo = a.W; a.Cout = d->cout; a.ypitch = y->pitch;
    a.ks = 1; a.stride = 1; a.pad = 0; a.act = d->act; a.ntaps = 1;
    a.oH = a.Ho; a.oW = a.Wo; a.omul = 1;
    a.M = (int)M;
    a.Kpad = y3_filter_kpad(d->cin, 1);
    a.x_bytes = (unsigned)ext(u_in); a.y_bytes = (unsigned)ext(y);
    a.w_bytes = (unsigned)((long long)y3_filter_rows(d->cout) * a.Kpad * 2);
    a.in_scale = in_scale; a.in_shift = in_shift; a.in_act = in_act;
    a.in_res = in_res ? in_res->data : nullptr; a.in_rpitch = in_res ? in_res->pitch : 0; a.in_r_bytes = in_res ? (unsigned)ext(in_res) : 0u;
    a.in_y = y_in->data; a.in_ypitch = y_in->pitch; a.in_y_bytes = (unsigned)ext(y_in);
    if (!s1_plan(a, p.s1, s1_in(a))) Y3_FAIL("y3_conv2d_fwd_bnin: shape not covered (cin %d, cout %d)", d->cin, d->cout);
    return plan_s1(a, p);
}

extern "C" int64_t y3_conv2d_fwd_bnin_rows(const y3_conv_desc* d, const y3_tensor* u_in, const y3_tensor* y_in, const y3_tensor* y, int32_t has_shortcut) {
    y3_tensor r;
    if (has_shortcut && y_in) { r = *y_in; r.data = (void*)g_dummy; }
    ConvArgs a;
    ConvPlan p;
    if (bnin_fill(d, u_in, g_dummy, g_dummy, Y3_ACT_NONE, has_shortcut ? &r : nullptr, y_in, (const void*)g_dummy, g_dummy, y, a, p)) return -1;
    return p.rows();
}

extern "C" int y3_conv2d_fwd_bnin_stats(const y3_conv_desc* d, const y3_tensor* u_in, const float* in_scale, const float* in_shift, int32_t in_act, const y3_tensor* in_shortcut,
                                        const y3_tensor* y_in, const void* filt, const float* bias, const y3_tensor* y, float* stat_rows, int64_t capacity_rows, int64_t* n_rows,
                                        void* stream) {
    if (!in_scale || !in_shift || !filt || !bias || !n_rows) Y3_FAIL("y3_conv2d_fwd_bnin_stats: null argument");
    ConvArgs a;
    ConvPlan p;
    if (bnin_fill(d, u_in, in_scale, in_shift, in_act, in_shortcut, y_in, filt, bias, y, a, p)) return -1;
    const int64_t rows = p.rows();
    *n_rows = rows;
    if (stat_rows) {
        if (capacity_rows < rows) Y3_FAIL("y3_conv2d_fwd_bnin_stats: statistics buffer holds %lld rows, the launch writes %lld", (long long)capacity_rows, (long long)rows);
        a.stats = stat_rows;
    }
    launch_begin(a, p);
    return d->dtype == Y3_F16 ? launch_s1<f16_t>(a, p.s1, (hipStream_t)stream) : launch_s1<bf16_t>(a, p.s1, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------------------------------------------------
// Data gradient of a 3x3 stride-2 pad-1 convolution without the 4x zero-tap waste of the dilated form: the gradient
// pixels split into four parity classes (hi%2, wi%2); class (ph, pw) only ever meets the taps kh = 1 (ph = 0) or
// kh in {0, 2} (ph = 1), likewise for kw -> 1 + 2 + 2 + 4 = 9 taps in total, i.e. exactly the forward MACs.  Each class is
// a stride-1 conv of du with its own small tap table and filter bank, written to every second pixel of the gradient.
// (S2Class, s2_class and the banks' geometry: filter_bank.h)
namespace {
// the four classes as one launch of the v3 tile that the plan of class `big`, the one with the most taps, chose
template <typename T> int launch_v3_quad(const ConvArgs* cls, int big, const ConvPlan& p, hipStream_t st) {
    ConvArgs lead = cls[big];
    launch_begin(lead, p);
    g_last_variant = "v3_quad";
    return conv_launch<T>(lead, p, st, cls);
}

}  // namespace

#ifdef Y3_TIMELINE
extern "C" void y3_debug_timeline(void* buf) { g_timeline = (unsigned long long*)buf; }
#endif

extern "C" int y3_conv2d_dgrad_s2(int32_t dtype, const y3_tensor* du, const void* packed4, const y3_tensor* residual, const y3_tensor* gx, void* stream) {
    if (!du || !packed4 || !gx) Y3_FAIL("y3_conv2d_dgrad_s2: null argument");
    if (dtype != Y3_F16 && dtype != Y3_BF16) Y3_FAIL("y3_conv2d_dgrad_s2: f16/bf16 only (fp32 uses the dilated form)");
    const int H = gx->h, W = gx->w;
    if (gx->n != du->n || du->h != (H - 1) / 2 + 1 || du->w != (W - 1) / 2 + 1) Y3_FAIL("y3_conv2d_dgrad_s2: (%d,%d) is not the stride-2 output of (%d,%d)", du->h, du->w, H, W);
    if ((du->c % 8) || (gx->c % 8) || (du->pitch % 8) || (gx->pitch % 8) || ((uintptr_t)du->data & 15) || ((uintptr_t)gx->data & 15) || ((uintptr_t)packed4 & 15))
        Y3_FAIL("y3_conv2d_dgrad_s2: alignment");
    if (residual && (residual->h != H || residual->w != W || residual->c != gx->c || (residual->pitch % 8))) Y3_FAIL("y3_conv2d_dgrad_s2: residual shape");
    if ((long long)gx->n * H * W > 0x7fffffffLL) Y3_FAIL("y3_conv2d_dgrad_s2: too many gradient pixels");
    hipStream_t st = (hipStream_t)stream;
    const int cout = du->c, cin = gx->c;
    const S2Banks banks = s2_banks(cout, cin);   // filter_bank.h: what y3_pack_filter_dgrad_s2 wrote
    ConvArgs cls[4];
    bool live[4];
    for (int ph = 0; ph < 2; ++ph)
        for (int pw = 0; pw < 2; ++pw) {
            const S2Class c = s2_class(ph, pw);
            const int ntaps = c.nh * c.nw;
            const int kpad = banks.kpad[ph * 2 + pw];
            const int Hc = (H - ph + 1) / 2, Wc = (W - pw + 1) / 2;
            const size_t bank = (size_t)banks.rows * kpad, off = banks.off[ph * 2 + pw];
            ConvArgs& a = cls[ph * 2 + pw];
            live[ph * 2 + pw] = Hc > 0 && Wc > 0;
            memset(&a, 0, sizeof(a));
            if (Hc > 0 && Wc > 0) {
                a.x = du->data; a.w = (const char*)packed4 + off * 2; a.bias = nullptr; a.res = residual ? residual->data : nullptr; a.y = gx->data;
                a.N = du->n; a.H = du->h; a.W = du->w; a.Cin = cout; a.xpitch = du->pitch;
                a.Ho = Hc; a.Wo = Wc; a.Cout = cin; a.ypitch = gx->pitch; a.rpitch = residual ? residual->pitch : 0;
                a.ks = 3; a.stride = 1; a.pad = 0; a.act = Y3_ACT_NONE; a.ups = 0; a.dil_shift = 0;
                a.M = du->n * Hc * Wc;
                a.Kpad = kpad;
                a.ntaps = ntaps;
                for (int ih = 0; ih < c.nh; ++ih)
                    for (int iw = 0; iw < c.nw; ++iw) { a.tdh[ih * c.nw + iw] = (signed char)c.dh[ih]; a.tdw[ih * c.nw + iw] = (signed char)c.dw[iw]; }
                a.oH = H; a.oW = W; a.omul = 2; a.ooh = ph; a.oow = pw;
                const long long xb = (((long long)du->n * du->h * du->w - 1) * du->pitch + du->c) * 2, wb = (long long)bank * 2;
                a.x_bytes = xb < 0x7fffffffLL ? (unsigned)xb : 0u;
                a.w_bytes = wb < 0x7fffffffLL ? (unsigned)wb : 0u;
                const long long yb = (((long long)gx->n * H * W - 1) * gx->pitch + gx->c) * 2, rb = residual ? (((long long)gx->n * H * W - 1) * residual->pitch + residual->c) * 2 : 0;
                a.y_bytes = yb < 0x7fffffffLL ? (unsigned)yb : 0u;
                a.r_bytes = rb < 0x7fffffffLL ? (unsigned)rb : 0u;
                if (!a.x_bytes || !a.w_bytes || !a.y_bytes || (residual && !a.r_bytes)) Y3_FAIL("y3_conv2d_dgrad_s2: tensor too large");
            }
        }
    // all four classes in ONE launch when they share the geometry (even H and W) and the dispatcher picks a v3 tile for the class with
    // the longest K loop (the 4-tap class: its variant suits the shorter ones); knob "dgrad_quad" = 0 keeps the four launches (A/B)
    const bool quad_on = y3_knob(Y3K_DGRAD_QUAD) != 0;
    bool quad = quad_on && live[0] && live[1] && live[2] && live[3] && cls[0].M == cls[3].M && cls[1].M == cls[3].M && cls[2].M == cls[3].M;
    if (quad) {
        CsPlan sp;
        if (cq_plan(cls, sp)) return dtype == Y3_F16 ? launch_cq<f16_t>(cls, sp, st) : launch_cq<bf16_t>(cls, sp, st);   // conv_strip.h: du rows staged once for the nine (tap, class) pairs
        int big = 0;
        for (int i = 1; i < 4; ++i)
            if (cls[i].ntaps > cls[big].ntaps) big = i;
        ConvPlan p;
        if (const int rc = conv_decide(cls[big], p)) return rc;
        if (p.is_v3() && ((long long)p.n_ct * p.n_pt + 7) / 8 * 32 <= 0x7fffffffLL) return dtype == Y3_F16 ? launch_v3_quad<f16_t>(cls, big, p, st) : launch_v3_quad<bf16_t>(cls, big, p, st);
    }
    for (int i = 0; i < 4; ++i)
        if (live[i]) {
            ConvPlan p;
            if (const int rc = conv_decide(cls[i], p)) return rc;
            if (const int rc = conv_launch_as(dtype, cls[i], p, st)) return rc;
        }
    return 0;
}
