// Every filter-bank packer of libyolov3_hip.so: OIHW fp32 weights -> the layouts of filter_bank.h.
//   destination-indexed (a thread per bank element, the WHOLE bank written, padding = 0): y3_pack_filter, _dgrad, _pair, _dgrad_s2, _stem
//   source-indexed tiles, many layers per launch (ONLY weight elements written, the caller zero-fills a bank once): y3_pack_filter_jobs, y3_fold_pack_jobs
#include "y3_common.h"

namespace {

// ---- destination-indexed: N banks of one layer's weights per launch, the grid sized by the largest -------------------------------------------------------------
template <int N> struct BankSet {
    y3_bank bank[N];
    void* dst[N];
};

template <typename T, int N>
__global__ void pack_banks_kernel(const float* __restrict__ src, const BankSet<N> s) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const y3_bank& b = s.bank[i];
        const long long total = (long long)b.rows * b.kpad;
        if (idx >= total) continue;
        const int k = (int)(idx % b.kpad), row = (int)(idx / b.kpad);
        const long long o = y3_bank_source(b, row, k);
        const T v = from_f32<T>(o >= 0 ? src[o] : 0.0f);
        T* __restrict__ dst = (T*)s.dst[i];
        dst[idx] = v;
        if (b.frag && k < b.ntaps * b.cpt) dst[total + y3_frag_index(row, k, b.cpt)] = v;   // the copy conv_v10.h reads
    }
}

template <int N> int launch_pack_banks(const char* who, int dtype, bool f32_too, const float* w, const BankSet<N>& s, hipStream_t st) {
    long long total = 0;
    for (int i = 0; i < N; ++i) {
        const long long t = (long long)s.bank[i].rows * s.bank[i].kpad;
        total = t > total ? t : total;
    }
    const dim3 grid((unsigned)((total + 255) / 256));
    switch (dtype) {
        case Y3_F16: hipLaunchKernelGGL((pack_banks_kernel<f16_t, N>), grid, dim3(256), 0, st, w, s); break;
        case Y3_BF16: hipLaunchKernelGGL((pack_banks_kernel<bf16_t, N>), grid, dim3(256), 0, st, w, s); break;
        case Y3_F32:
            if (f32_too) { hipLaunchKernelGGL((pack_banks_kernel<float, N>), grid, dim3(256), 0, st, w, s); break; }
            [[fallthrough]];
        default:
            if (f32_too) Y3_FAIL("%s: bad dtype %d", who, dtype);
            Y3_FAIL("%s: f16/bf16 only", who);
    }
    Y3_CHECK_LAUNCH();
    return 0;
}
bool taps_fit(int ks) { return ks >= 1 && ks <= 3; }   // what the tap table of y3_bank holds (the conv kernels take 1 and 3)

// ---- source-indexed tiles ----------------------------------------------------------------------------------------------------------------------------------------
// Every layer's banks in ONE launch: the training step re-packs all filters each step (the fp32 master weights moved); 75 pack launches of 4-40 us (0.8 ms per
// batch-64 step, most of it launch-to-launch latency) became one in round 3.  Round 5: SOURCE-indexed tiles.  The destination-indexed form above gathered the weights
// with a stride of 9 floats for the forward bank and of 9 Cin floats for the data-gradient bank -- 1.6 GB of reads for 248 MB of weights, 0.54 ms.  Now a block owns a
// 32-filter x 32-channel tile: it reads the tile's 32 x (32 k k) floats as 32 contiguous runs, keeps them as T in LDS ([tap][filter][channel]) and writes the
// destinations -- forward bank (32 consecutive channels of a (filter, tap) = 64 bytes), data-gradient bank (32 consecutive filters of a (channel, flipped tap)), and the
// fragment-ordered copies of either -- from there.  ONLY the elements that come from a weight are written: row padding (filters / channels beyond the source's) and K
// padding stay what they are, so the caller zero-fills a bank ONCE when it allocates it (ops.PackJobs and engine.FoldPackJobs do).
constexpr int PT = 32;   // tile edge: y3_pack_job_blocks counts PT x PT tiles
template <typename T> using PackTile = T[9][PT][PT + 2];   // (34: the transposed read of the data-gradient pass walks the filter index: 17 dwords apart)

// the job that owns this block: a binary search over the jobs' first block (wave-uniform scalar loads)
template <typename J> Y3_DEV J find_job(const J* __restrict__ jobs, int n_jobs) {
    int lo = 0, hi = n_jobs - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (jobs[mid].first_block <= (int)blockIdx.x) lo = mid; else hi = mid - 1;
    }
    return jobs[lo];
}
// the block's tile origin; false for a tile of padding only (uniform)
template <typename J> Y3_DEV bool job_tile(const J& j, int& co0, int& ci0) {
    const int n_tci = (j.cin + PT - 1) / PT;
    const int t = (int)blockIdx.x - j.first_block;
    co0 = (t / n_tci) * PT; ci0 = (t % n_tci) * PT;
    return co0 < j.cout_src && ci0 < j.cin_src;
}
// weights -> LDS as T, times the filter's scale[0 .. PT) when given
template <typename T, typename J> Y3_DEV void tile_load(PackTile<T>& tile, const J& j, int co0, int ci0, const float* scale) {
    const float* __restrict__ src = j.w;
    const int KK = j.ksize * j.ksize;
    for (int e = threadIdx.x; e < PT * PT * KK; e += 256) {
        const int co_l = e / (PT * KK), r = e - co_l * (PT * KK);
        const int ci_l = r / KK, tap = r - ci_l * KK;
        const int co = co0 + co_l, ci = ci0 + ci_l;
        float v = 0.0f;
        if (co < j.cout_src && ci < j.cin_src) {
            v = src[((long long)co * j.cin_src + ci) * KK + tap];
            if (scale) v = scale[co_l] * v;
        }
        tile[tap][co_l][ci_l] = from_f32<T>(v);
    }
    __syncthreads();
}
template <typename T, typename J> Y3_DEV void tile_store_fwd(const PackTile<T>& tile, const J& j, int co0, int ci0, T* __restrict__ dst) {
    const int KK = j.ksize * j.ksize, kpad = y3_filter_kpad(j.cin, j.ksize);
    const long long total = (long long)y3_filter_rows(j.cout) * kpad;
    const bool frag = y3_filter_has_frag(j.cout, j.cin, j.ksize);
    for (int e = threadIdx.x; e < PT * PT * KK; e += 256) {
        const int ci_l = e & 31, co_l = (e >> 5) & 31, tap = e >> 10;
        const int co = co0 + co_l, ci = ci0 + ci_l;
        if (co < j.cout_src && ci < j.cin_src) {
            const T v = tile[tap][co_l][ci_l];
            const int k = tap * j.cin + ci;
            dst[(long long)co * kpad + k] = v;
            if (frag) dst[total + y3_frag_index(co, k, j.cin)] = v;   // the copy conv_v10.h reads
        }
    }
}
template <typename T, typename J> Y3_DEV void tile_store_dgrad(const PackTile<T>& tile, const J& j, int co0, int ci0, T* __restrict__ dst) {
    const int KK = j.ksize * j.ksize, kpad = y3_filter_kpad(j.cout, j.ksize);
    const long long total = (long long)y3_filter_rows(j.cin) * kpad;
    const bool frag = y3_filter_has_frag(j.cin, j.cout, j.ksize);
    for (int e = threadIdx.x; e < PT * PT * KK; e += 256) {
        const int co_l = e & 31, ci_l = (e >> 5) & 31, tap = e >> 10;
        const int co = co0 + co_l, ci = ci0 + ci_l;
        if (co < j.cout_src && ci < j.cin_src) {
            const T v = tile[tap][co_l][ci_l];
            const int k = (KK - 1 - tap) * j.cout + co;   // flipped tap (kh, kw) -> (ks - 1 - kh, ks - 1 - kw)
            dst[(long long)ci * kpad + k] = v;
            if (frag) dst[total + y3_frag_index(ci, k, j.cout)] = v;
        }
    }
}
// ksize 3, <= 4 channels (checked by the host mirror): one channel tile
template <typename T, typename J> Y3_DEV void tile_store_stem(const PackTile<T>& tile, const J& j, int co0, T* __restrict__ dst) {
    for (int e = threadIdx.x; e < PT * 4 * 9; e += 256) {
        const int c = e & 3, co_l = (e >> 2) & 31, tap = e >> 7;
        const int co = co0 + co_l;
        if (co < j.cout_src && c < j.cin_src) dst[y3_stem_index(co, tap / 3, tap % 3, c)] = tile[tap][co_l][c];
    }
}

template <typename T>
__global__ __launch_bounds__(256) void pack_filter_jobs_kernel(const y3_pack_job* __restrict__ jobs, int n_jobs) {
    __shared__ PackTile<T> tile;
    const y3_pack_job j = find_job(jobs, n_jobs);
    int co0, ci0;
    if (!job_tile(j, co0, ci0)) return;
    tile_load<T>(tile, j, co0, ci0, nullptr);
    if (j.packed_fwd) tile_store_fwd<T>(tile, j, co0, ci0, (T*)j.packed_fwd);
    if (j.packed_dgrad) tile_store_dgrad<T>(tile, j, co0, ci0, (T*)j.packed_dgrad);
}

// ---- inference plans: Conv + BatchNorm fold and pack of EVERY layer in one launch (y3_fold_pack_jobs) ------------------------------------------------------------
// The algebra of upstream fuse_conv_and_bn as yolov3_amd/engine.py::_fold evaluates it with torch, operation for operation: IEEE sqrt and division, every product and
// sum rounded on its own (no FMA contraction in these two functions, whatever the file is built with) -- the banks equal the ones _fold + y3_pack_filter write, bit for bit.
__device__ __forceinline__ float fold_scale(float gamma, float var, float eps) {
#pragma clang fp contract(off)
    return gamma / sqrtf(eps + var);
}
__device__ __forceinline__ float fold_bias(float scale, float b, float gamma, float beta, float mean, float var, float eps) {
#pragma clang fp contract(off)
    const float gm = gamma * mean;
    const float b_bn = beta - gm / sqrtf(var + eps);
    const float sb = scale * b;
    return sb + b_bn;
}

// The tiles of pack_filter_jobs_kernel; the weights are scaled by their filter's BatchNorm factor on the way into LDS and leave in the layout of y3_pack_filter (+ the
// fragment-ordered copy) or, for a `stem` job, of y3_pack_filter_stem.  The block of channel tile 0 also writes its 32 entries of the fp32 bias vector.  Only elements
// that come from a weight are written: banks and bias vectors are zero-filled once by the caller.
template <typename T>
__global__ __launch_bounds__(256) void fold_pack_jobs_kernel(const y3_fold_pack_job* __restrict__ jobs, int n_jobs) {
    __shared__ PackTile<T> tile;
    __shared__ float sc[PT];
    const y3_fold_pack_job j = find_job(jobs, n_jobs);
    int co0, ci0;
    if (!job_tile(j, co0, ci0)) return;
    const bool bn = j.bn_gamma != nullptr;
    if (threadIdx.x < PT) {
        const int co = co0 + threadIdx.x;
        float s = 1.0f;
        if (co < j.cout_src) {
            if (bn) s = fold_scale(j.bn_gamma[co], j.bn_var[co], j.bn_eps);
            if (ci0 == 0) {
                const float b = j.conv_bias ? j.conv_bias[co] : 0.0f;
                j.bias[co] = bn ? fold_bias(s, b, j.bn_gamma[co], j.bn_beta[co], j.bn_mean[co], j.bn_var[co], j.bn_eps) : b;
            }
        }
        sc[threadIdx.x] = s;
    }
    __syncthreads();
    tile_load<T>(tile, j, co0, ci0, bn ? sc : nullptr);
    if (j.stem) tile_store_stem<T>(tile, j, co0, (T*)j.packed);
    else tile_store_fwd<T>(tile, j, co0, ci0, (T*)j.packed);
}

}  // namespace

extern "C" size_t y3_packed_filter_elems(int32_t cout, int32_t cin, int32_t ksize) { return y3_filter_elems(cout, cin, ksize); }

extern "C" int y3_pack_filter(const float* w, int32_t cout_src, int32_t cin_src, int32_t ks, int32_t cout, int32_t cin, int32_t dtype, void* packed, void* stream) {
    if (!w || !packed) Y3_FAIL("y3_pack_filter: null pointer");
    if (cout < cout_src || cin < cin_src || (cin % 8) != 0) Y3_FAIL("y3_pack_filter: bad padded sizes cout=%d cin=%d", cout, cin);
    if (!taps_fit(ks)) Y3_FAIL("y3_pack_filter: ksize %d unsupported", ks);
    const BankSet<1> s = {{y3_bank_fwd(cout_src, cin_src, ks, cout, cin)}, {packed}};
    return launch_pack_banks("y3_pack_filter", dtype, true, w, s, (hipStream_t)stream);
}

extern "C" size_t y3_packed_filter_stem_elems(int32_t cout) { return (size_t)y3_stem_rows(cout) * Y3_STEM_KPAD; }

extern "C" int y3_pack_filter_stem(const float* w, int32_t cout_src, int32_t cin_src, int32_t cout, int32_t dtype, void* packed, void* stream) {
    if (!w || !packed) Y3_FAIL("y3_pack_filter_stem: null pointer");
    if (cin_src < 1 || cin_src > 4 || cout < cout_src) Y3_FAIL("y3_pack_filter_stem: needs 1..4 input channels and cout >= cout_src");
    const BankSet<1> s = {{y3_bank_stem(cout_src, cin_src, cout)}, {packed}};
    return launch_pack_banks("y3_pack_filter_stem", dtype, false, w, s, (hipStream_t)stream);
}

extern "C" int y3_pack_filter_dgrad(const float* w, int32_t cout_src, int32_t cin_src, int32_t ks, int32_t cout, int32_t cin, int32_t dtype, void* packed, void* stream) {
    if (!w || !packed) Y3_FAIL("y3_pack_filter_dgrad: null pointer");
    if (cout < cout_src || cin < cin_src || (cout % 8) != 0 || (cin % 8) != 0) Y3_FAIL("y3_pack_filter_dgrad: bad padded sizes");
    if (!taps_fit(ks)) Y3_FAIL("y3_pack_filter_dgrad: ksize %d unsupported", ks);
    const BankSet<1> s = {{y3_bank_dgrad(cout_src, cin_src, ks, cout, cin)}, {packed}};
    return launch_pack_banks("y3_pack_filter_dgrad", dtype, true, w, s, (hipStream_t)stream);
}

// y3_pack_filter and y3_pack_filter_dgrad of one layer in one launch
extern "C" int y3_pack_filter_pair(const float* w, int32_t cout_src, int32_t cin_src, int32_t ks, int32_t cout, int32_t cin, int32_t dtype, void* packed_fwd, void* packed_dgrad,
                                   void* stream) {
    if (!w || !packed_fwd || !packed_dgrad) Y3_FAIL("y3_pack_filter_pair: null pointer");
    if (cout < cout_src || cin < cin_src || (cout % 8) != 0 || (cin % 8) != 0) Y3_FAIL("y3_pack_filter_pair: bad padded sizes");
    if (!taps_fit(ks)) Y3_FAIL("y3_pack_filter_pair: ksize %d unsupported", ks);
    const BankSet<2> s = {{y3_bank_fwd(cout_src, cin_src, ks, cout, cin), y3_bank_dgrad(cout_src, cin_src, ks, cout, cin)}, {packed_fwd, packed_dgrad}};
    return launch_pack_banks("y3_pack_filter_pair", dtype, false, w, s, (hipStream_t)stream);
}

extern "C" size_t y3_packed_filter_dgrad_s2_elems(int32_t cout, int32_t cin) { return s2_banks(cout, cin).total; }

// one launch per parity class
extern "C" int y3_pack_filter_dgrad_s2(const float* w, int32_t cout_src, int32_t cin_src, int32_t cout, int32_t cin, int32_t dtype, void* packed, void* stream) {
    if (!w || !packed) Y3_FAIL("y3_pack_filter_dgrad_s2: null pointer");
    if (cout < cout_src || cin < cin_src || (cout % 8) || (cin % 8)) Y3_FAIL("y3_pack_filter_dgrad_s2: bad padded sizes");
    const S2Banks g = s2_banks(cout, cin);
    const int esz = dtype == Y3_F32 ? 4 : 2;
    for (int i = 0; i < 4; ++i) {
        const BankSet<1> s = {{y3_bank_dgrad_s2(cout_src, cin_src, cout, cin, i)}, {(char*)packed + g.off[i] * esz}};
        if (const int rc = launch_pack_banks("y3_pack_filter_dgrad_s2", dtype, false, w, s, (hipStream_t)stream)) return rc;
    }
    return 0;
}

// blocks a job of y3_pack_filter_jobs occupies (the caller lays the jobs out back to back: first_block = running sum)
extern "C" int64_t y3_pack_job_blocks(int32_t ksize, int32_t cout, int32_t cin, int32_t want_fwd, int32_t want_dgrad) {
    (void)ksize; (void)want_fwd; (void)want_dgrad;
    return (int64_t)((cout + PT - 1) / PT) * ((cin + PT - 1) / PT);   // one block per 32-filter x 32-channel tile of the weights
}

extern "C" int y3_pack_filter_jobs(const y3_pack_job* jobs_device, int32_t n_jobs, int64_t total_blocks, int32_t dtype, void* stream) {
    if (!jobs_device || n_jobs <= 0 || total_blocks <= 0 || total_blocks > 0x7fffffffLL) Y3_FAIL("y3_pack_filter_jobs: bad argument");
    hipStream_t st = (hipStream_t)stream;
    if (dtype == Y3_F16) hipLaunchKernelGGL((pack_filter_jobs_kernel<f16_t>), dim3((unsigned)total_blocks), dim3(256), 0, st, jobs_device, n_jobs);
    else if (dtype == Y3_BF16) hipLaunchKernelGGL((pack_filter_jobs_kernel<bf16_t>), dim3((unsigned)total_blocks), dim3(256), 0, st, jobs_device, n_jobs);
    else Y3_FAIL("y3_pack_filter_jobs: f16/bf16 only");
    Y3_CHECK_LAUNCH();
    return 0;
}

// One launch for a whole model's inference banks: see fold_pack_jobs_kernel.  The table is DEVICE memory and cannot be inspected here: its geometry is the host mirror's
// (yolov3_amd/engine.py::FoldPackJobs) to get right.
extern "C" int y3_fold_pack_jobs(const y3_fold_pack_job* jobs_device, int32_t n_jobs, int64_t total_blocks, int32_t dtype, void* stream) {
    if (!jobs_device) Y3_FAIL("y3_fold_pack_jobs: null job table");
    if (n_jobs <= 0 || total_blocks <= 0 || total_blocks > 0x7fffffffLL) Y3_FAIL("y3_fold_pack_jobs: n_jobs %d and total_blocks %lld must be positive (and fit a grid)", (int)n_jobs, (long long)total_blocks);
    hipStream_t st = (hipStream_t)stream;
    switch (dtype) {
        case Y3_F16: hipLaunchKernelGGL((fold_pack_jobs_kernel<f16_t>), dim3((unsigned)total_blocks), dim3(256), 0, st, jobs_device, n_jobs); break;
        case Y3_BF16: hipLaunchKernelGGL((fold_pack_jobs_kernel<bf16_t>), dim3((unsigned)total_blocks), dim3(256), 0, st, jobs_device, n_jobs); break;
        case Y3_F32: hipLaunchKernelGGL((fold_pack_jobs_kernel<float>), dim3((unsigned)total_blocks), dim3(256), 0, st, jobs_device, n_jobs); break;
        default: Y3_FAIL("y3_fold_pack_jobs: bad dtype %d (f16 / bf16 / f32)", (int)dtype);
    }
    Y3_CHECK_LAUNCH();
    return 0;
}
