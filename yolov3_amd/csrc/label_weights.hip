// Class and image weights of --image-weights training on gfx950: what reference train.py:333 and :360-363 run on the host with one np.bincount per image --
//   * labels_to_class_weights (utils/general.py:543-561): the class histogram over every label          -> label_histogram_kernel (the nc-element tail stays on the host)
//   * labels_to_image_weights (:564-568): iw[i] = sum_c cw[c] count[i][c]                                 -> image_weights_kernel, one wave per image
//   * random.choices(range(n), weights=iw, k=k): accumulate, then bisect_right(cum, u total, 0, n - 1)    -> scan_* kernels and choices_kernel (the uniforms come from the host)
// A class id is the label's first column truncated toward zero, as astype(int) truncates it; an id outside [0, nc) is counted into an error word, never used as an index.
// Counts are integers (LDS bins per block, one global add per non-empty bin): independent of order.  Every fp64 sum has ONE order that the launch geometry cannot change:
//   image weights: lane l of the image's wave adds cw[id_j] for j = first + l, first + l + 64, ... in ascending j; the 64 lane sums are combined by the xor butterfly
//                  with the distances 32, 16, 8, 4, 2, 1 (both partners form the same commutative sum, so every lane ends with the same bits);
//   prefix sum:    chunks of SCAN_CHUNK = 2048 weights, 8 consecutive ones per thread.  A thread adds its 8 in ascending order; the 256 thread sums are scanned by
//                  Hillis-Steele steps of distance 1, 2, ..., 128; the chunk totals are scanned the same way, 256 at a time, with a running carry; then
//                  cum[i] = ((carry of the chunk + exclusive prefix of the thread) + x_first) + ... + x_i.
// Results are therefore run-to-run bit-identical.  The sums differ from NumPy's / itertools.accumulate's serial order by at most (terms) 2^-53 relative for weights of one sign.
// Built with -ffp-contract=off (nothing here multiplies and adds, the flag keeps it so).
#include "y3_common.h"

#include <math.h>

namespace {

constexpr int BT = 256;              // threads of a block
constexpr int WAVE = 64;
constexpr int HIST_MAX_NC = 4096;    // LDS bins of the histogram (16 KB)
constexpr int HIST_MAX_BLOCKS = 1024;
constexpr int IW_MAX_BLOCKS = 1 << 16;
constexpr int SCAN_PER_THREAD = 8;
constexpr int SCAN_CHUNK = BT * SCAN_PER_THREAD;

// the label's class: the fp32 id truncated toward zero when that lies in [0, nc), else false (NaN included)
Y3_DEV bool class_id(float f, int nc, int& c) {
    if (!(f > -1.0f && f < (float)nc)) return false;
    c = (int)f;
    return true;
}

// ---- class histogram ---------------------------------------------------------------------------------------------------------------
// counts[c] += labels of class c, counts[nc] += ids outside [0, nc)
__global__ __launch_bounds__(BT) void label_histogram_kernel(const float* __restrict__ cls, int stride, long long n, int* __restrict__ counts, int nc) {
    __shared__ int s_bins[HIST_MAX_NC + 1];
    const int tid = threadIdx.x;
    for (int b = tid; b <= nc; b += BT) s_bins[b] = 0;
    __syncthreads();
    for (long long i = (long long)blockIdx.x * BT + tid; i < n; i += (long long)gridDim.x * BT) {
        int c;
        atomicAdd(&s_bins[class_id(cls[i * stride], nc, c) ? c : nc], 1);
    }
    __syncthreads();
    for (int b = tid; b <= nc; b += BT) {
        const int v = s_bins[b];
        if (v) atomicAdd(counts + b, v);
    }
}

// ---- image weights -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BT) void image_weights_kernel(const float* __restrict__ cls, long long N, const long long* __restrict__ offsets, long long n_img,
                                                            const double* __restrict__ cw, int nc, double* __restrict__ iw) {
    const int lane = threadIdx.x & (WAVE - 1);
    const long long waves = (long long)gridDim.x * (BT / WAVE);
    for (long long img = (long long)blockIdx.x * (BT / WAVE) + (threadIdx.x / WAVE); img < n_img; img += waves) {   // (uniform over the wave)
        long long beg = offsets[img], end = offsets[img + 1];
        beg = beg < 0 ? 0 : (beg > N ? N : beg);   // a table that does not describe cls reads nothing outside it
        end = end < beg ? beg : (end > N ? N : end);
        double acc = 0.0;
        for (long long j = beg + lane; j < end; j += WAVE) {
            int c;
            if (class_id(cls[j], nc, c)) acc += cw[c];
        }
        for (int d = WAVE / 2; d > 0; d >>= 1) acc += __shfl_xor(acc, d, WAVE);
        if (lane == 0) iw[img] = acc;
    }
}

// ---- prefix sum ----------------------------------------------------------------------------------------------------------------------
// inclusive Hillis-Steele scan of the block's BT values; s[] holds the inclusive prefixes afterwards
Y3_DEV double block_scan(double v, double* s) {
    const int tid = threadIdx.x;
    __syncthreads();
    s[tid] = v;
    __syncthreads();
    for (int d = 1; d < BT; d <<= 1) {
        const double t = tid >= d ? s[tid - d] : 0.0;
        __syncthreads();
        if (tid >= d) s[tid] += t;
        __syncthreads();
    }
    return s[tid];
}

// the thread's SCAN_PER_THREAD consecutive weights of chunk blockIdx.x (0.0 past the end: adding it is exact) and their sum in ascending order
Y3_DEV double load_run(const double* __restrict__ w, long long n, double (&x)[SCAN_PER_THREAD]) {
    const long long first = (long long)blockIdx.x * SCAN_CHUNK + (long long)threadIdx.x * SCAN_PER_THREAD;
    double v = 0.0;
#pragma unroll
    for (int e = 0; e < SCAN_PER_THREAD; ++e) {
        x[e] = first + e < n ? w[first + e] : 0.0;
        v += x[e];
    }
    return v;
}

__global__ __launch_bounds__(BT) void scan_chunk_totals_kernel(const double* __restrict__ w, long long n, double* __restrict__ carries) {
    __shared__ double s[BT];
    double x[SCAN_PER_THREAD];
    const double incl = block_scan(load_run(w, n, x), s);
    if (threadIdx.x == BT - 1) carries[blockIdx.x] = incl;
}

// chunk totals -> the exclusive prefix of every chunk, in place, by ONE block
__global__ __launch_bounds__(BT) void scan_carries_kernel(double* __restrict__ carries, long long nchunks) {
    __shared__ double s[BT];
    const int tid = threadIdx.x;
    double running = 0.0;
    for (long long base = 0; base < nchunks; base += BT) {
        const long long i = base + tid;
        block_scan(i < nchunks ? carries[i] : 0.0, s);
        const double excl = tid ? s[tid - 1] : 0.0;
        if (i < nchunks) carries[i] = running + excl;
        running += s[BT - 1];   // (the next scan's leading barrier keeps s[] until every thread has read it)
    }
}

__global__ __launch_bounds__(BT) void scan_write_kernel(const double* __restrict__ w, long long n, const double* __restrict__ carries, double* __restrict__ cum) {
    __shared__ double s[BT];
    const int tid = threadIdx.x;
    double x[SCAN_PER_THREAD];
    block_scan(load_run(w, n, x), s);
    const double excl = tid ? s[tid - 1] : 0.0;
    double running = blockIdx.x ? carries[blockIdx.x] + excl : excl;
    const long long first = (long long)blockIdx.x * SCAN_CHUNK + (long long)tid * SCAN_PER_THREAD;
#pragma unroll
    for (int e = 0; e < SCAN_PER_THREAD; ++e) {
        if (first + e < n) {
            running += x[e];
            cum[first + e] = running;
        }
    }
}

// ---- the k searches ------------------------------------------------------------------------------------------------------------------
// out[j] = bisect_right(cum, u[j] * total, 0, n - 1), total = cum[n - 1] + 0.0; out[k] = 0, 1 (total <= 0) or 2 (total not finite)
__global__ __launch_bounds__(BT) void choices_kernel(const double* __restrict__ cum, long long n, const double* __restrict__ u, long long k, long long* __restrict__ out) {
    const long long j = (long long)blockIdx.x * BT + threadIdx.x;
    const double total = cum[n - 1] + 0.0;
    if (j == 0) out[k] = total <= 0.0 ? 1 : (isfinite(total) ? 0 : 2);
    if (j >= k) return;
    const double x = u[j] * total;
    long long lo = 0, hi = n - 1;
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (x < cum[mid]) hi = mid;
        else lo = mid + 1;
    }
    out[j] = lo;
}

bool aligned8(const void* p) { return ((uintptr_t)p & 7) == 0; }
long long scan_chunks(long long n) { return (n + SCAN_CHUNK - 1) / SCAN_CHUNK; }

}  // namespace

extern "C" int y3_label_histogram(const float* cls, int32_t stride, int64_t n, int32_t* counts, int32_t nc, void* stream) {
    if (!counts || (n > 0 && !cls)) Y3_FAIL("y3_label_histogram: null argument");
    if (n < 0 || n > 0x7fffffffLL || stride < 1) Y3_FAIL("y3_label_histogram: bad geometry (n %lld in 0 .. 2^31 - 1, stride %d)", (long long)n, stride);
    if (nc < 1 || nc > HIST_MAX_NC) Y3_FAIL("y3_label_histogram: %d classes unsupported (1 .. %d)", nc, HIST_MAX_NC);
    hipStream_t st = (hipStream_t)stream;
    Y3_HIP(hipMemsetAsync(counts, 0, ((size_t)nc + 1) * sizeof(int32_t), st));
    if (n == 0) return 0;
    const long long blocks = (n + BT - 1) / BT;
    hipLaunchKernelGGL(label_histogram_kernel, dim3((unsigned)(blocks < HIST_MAX_BLOCKS ? blocks : HIST_MAX_BLOCKS)), dim3(BT), 0, st, cls, stride, (long long)n, counts, nc);
    Y3_CHECK_LAUNCH();
    return 0;
}

extern "C" int y3_image_weights(const float* cls, int64_t n_labels, const int64_t* offsets, int64_t n_img, const double* class_weights, int32_t nc, double* iw, void* stream) {
    if (!offsets || !class_weights || !iw || (n_labels > 0 && !cls)) Y3_FAIL("y3_image_weights: null argument");
    if (n_labels < 0 || n_labels > 0x7fffffffLL || n_img < 1 || n_img > 0x7fffffffLL)
        Y3_FAIL("y3_image_weights: bad geometry (%lld labels in 0 .. 2^31 - 1, %lld images in 1 .. 2^31 - 1)", (long long)n_labels, (long long)n_img);
    if (nc < 1 || nc > HIST_MAX_NC) Y3_FAIL("y3_image_weights: %d classes unsupported (1 .. %d)", nc, HIST_MAX_NC);
    if (!aligned8(offsets) || !aligned8(class_weights) || !aligned8(iw)) Y3_FAIL("y3_image_weights: the offsets and the fp64 buffers must be 8-byte aligned");
    const long long blocks = (n_img + (BT / WAVE) - 1) / (BT / WAVE);
    hipLaunchKernelGGL(image_weights_kernel, dim3((unsigned)(blocks < IW_MAX_BLOCKS ? blocks : IW_MAX_BLOCKS)), dim3(BT), 0, (hipStream_t)stream, cls, (long long)n_labels,
                       (const long long*)offsets, (long long)n_img, class_weights, nc, iw);
    Y3_CHECK_LAUNCH();
    return 0;
}

extern "C" size_t y3_weighted_choices_workspace_bytes(int64_t n) {
    if (n < 1 || n > 0x7fffffffLL) {
        y3_set_error("y3_weighted_choices_workspace_bytes: bad geometry (n %lld in 1 .. 2^31 - 1)", (long long)n);
        return 0;
    }
    return ((size_t)n + (size_t)scan_chunks(n)) * sizeof(double);   // the cumulative weights, then one carry per chunk
}

extern "C" int y3_weighted_choices(const double* weights, int64_t n, const double* u, int64_t k, int64_t* out, void* workspace, size_t workspace_bytes, void* stream) {
    if (!weights || !out || !workspace || (k > 0 && !u)) Y3_FAIL("y3_weighted_choices: null argument");
    if (n < 1 || n > 0x7fffffffLL || k < 0 || k > 0x7fffffffLL) Y3_FAIL("y3_weighted_choices: bad geometry (n %lld in 1 .. 2^31 - 1, k %lld in 0 .. 2^31 - 1)", (long long)n, (long long)k);
    if (!aligned8(weights) || !aligned8(u) || !aligned8(out) || !aligned8(workspace)) Y3_FAIL("y3_weighted_choices: the buffers and the workspace must be 8-byte aligned");
    const size_t need = y3_weighted_choices_workspace_bytes(n);
    if (workspace_bytes < need) Y3_FAIL("y3_weighted_choices: the workspace needs %zu bytes, %zu given", need, workspace_bytes);
    hipStream_t st = (hipStream_t)stream;
    double* cum = (double*)workspace;
    double* carries = cum + n;
    const long long chunks = scan_chunks(n);
    if (chunks > 1) {
        hipLaunchKernelGGL(scan_chunk_totals_kernel, dim3((unsigned)chunks), dim3(BT), 0, st, weights, (long long)n, carries);
        Y3_CHECK_LAUNCH();
        hipLaunchKernelGGL(scan_carries_kernel, dim3(1), dim3(BT), 0, st, carries, chunks);
        Y3_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(scan_write_kernel, dim3((unsigned)chunks), dim3(BT), 0, st, weights, (long long)n, (const double*)carries, cum);   // (one chunk: its carry is never read)
    Y3_CHECK_LAUNCH();
    const long long blocks = k > 0 ? (k + BT - 1) / BT : 1;   // k == 0 still writes the status word
    hipLaunchKernelGGL(choices_kernel, dim3((unsigned)blocks), dim3(BT), 0, st, (const double*)cum, (long long)n, u, (long long)k, (long long*)out);
    Y3_CHECK_LAUNCH();
    return 0;
}
