// Autoanchor on gfx950: what reference utils/autoanchor.py runs on the host before the first batch of a training run --
//   * check_anchors.metric / kmean_anchors.metric, anchor_fitness, print_results (:36-43, :90-116) -> anchor_metrics_kernel (six fp64 totals in one pass)
//   * the genetic loop of kmean_anchors (:150-160)                                                  -> anchor_evolve_kernel, one launch per generation, nothing read back
//   * scipy.cluster.vq.kmeans(wh / s, n, iter=30) (:141)                                             -> kmeans_step_kernel, one Lloyd iteration of R restarts per launch
// Per-point arithmetic is fp32 with IEEE-correctly rounded divisions in the reference's operation order (built with -ffp-contract=off, no fast-math): the
// per-element values are torch's CPU values bit for bit.  Every sum is fp64 in a fixed order -- a thread walks its points in ascending order, the block combines
// its threads in a fixed tree, the per-block partials are added in block-index order by the block that finishes last -- so results are run-to-run bit-identical.
// "Finishes last" is a ticket: thread 0 of a block stores the block's partials, releases them at agent scope and takes a ticket with an ordinary atomic add; the
// block that draws the last one acquires and reduces.  The ticket words are zeroed ahead of every launch sequence and reset by the reducer.
#include "y3_common.h"

namespace {

constexpr int BT = 256;           // threads of a block = points of a chunk
constexpr int MAX_N = 64;         // anchors / codes
constexpr int MAX_R = 64;         // k-means restarts of one launch (the frozen set is one 64-bit mask)
constexpr int MAX_BLOCKS = 1024;  // blocks over the points of the metric / fitness kernels (= partials the reducer adds serially)
constexpr int KM_BLOCKS = 256;    // blocks over the points per k-means restart
constexpr int NTOT = 6;           // totals of y3_anchor_metrics
constexpr size_t TICKET_BYTES = 256;   // MAX_R ticket words ahead of the partials

int point_blocks(long long N, int cap) {
    const long long b = (N + BT - 1) / BT;
    return (int)(b < cap ? b : cap);
}

// the block's partials are in memory: publish them and draw a ticket; true in every thread of the block that drew the last one
Y3_DEV bool last_block(unsigned* ticket, unsigned nblocks, int* s_flag) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the partials of every thread have left the wave before the barrier
    __syncthreads();
    if (threadIdx.x == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const unsigned t = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int last = t == nblocks - 1;
        if (last) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // the next launch of the stream starts from zero
        }
        *s_flag = last;
    }
    __syncthreads();
    const bool last = *s_flag != 0;
    if (last) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");   // every reading thread of the reducer, not only thread 0
    return last;
}

// fixed tree over the BT values of the block; the total is valid in thread 0
Y3_DEV double block_sum(double v, double* s) {
    const int tid = threadIdx.x;
    __syncthreads();
    s[tid] = v;
    __syncthreads();
    for (int d = BT / 2; d > 0; d >>= 1) {
        if (tid < d) s[tid] += s[tid + d];
        __syncthreads();
    }
    return s[0];
}

// x_j = min(min(r0, 1 / r0), min(r1, 1 / r1)), r = wh / k: the ratio metric of one label against one anchor, as torch.min(r, 1 / r).min(2)[0]
Y3_DEV float ratio_metric(float w, float h, float kw, float kh) {
    const float r0 = w / kw, r1 = h / kh;
    return fminf(fminf(r0, 1.0f / r0), fminf(r1, 1.0f / r1));
}

// ---- metrics -------------------------------------------------------------------------------------------------------------------
// totals[0] sum best [best > thr], [1] #(best > thr), [2] #(x > thr), [3] sum x, [4] sum best, [5] sum x [x > thr]
__global__ __launch_bounds__(BT) void anchor_metrics_kernel(const float* __restrict__ wh, long long N, const double* __restrict__ k, int n, float thr,
                                                             double* __restrict__ partials, unsigned* __restrict__ ticket, double* __restrict__ totals) {
    __shared__ float s_k[2 * MAX_N];
    __shared__ double s_red[BT];
    __shared__ int s_flag;
    const int tid = threadIdx.x;
    if (tid < 2 * n) s_k[tid] = (float)k[tid];   // torch.tensor(k, dtype=torch.float32)
    __syncthreads();
    double acc[NTOT] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (long long i = (long long)blockIdx.x * BT + tid; i < N; i += (long long)gridDim.x * BT) {
        const float w = wh[2 * i], h = wh[2 * i + 1];
        float best = 0.0f;
        for (int j = 0; j < n; ++j) {
            const float x = ratio_metric(w, h, s_k[2 * j], s_k[2 * j + 1]);
            best = j == 0 ? x : fmaxf(best, x);
            acc[3] += (double)x;
            if (x > thr) {
                acc[2] += 1.0;
                acc[5] += (double)x;
            }
        }
        acc[4] += (double)best;
        if (best > thr) {
            acc[0] += (double)best;
            acc[1] += 1.0;
        }
    }
    for (int q = 0; q < NTOT; ++q) {
        const double t = block_sum(acc[q], s_red);
        if (tid == 0) partials[(long long)blockIdx.x * NTOT + q] = t;
    }
    if (!last_block(ticket, gridDim.x, &s_flag)) return;
    if (tid < NTOT) {
        double t = 0.0;
        for (unsigned b = 0; b < gridDim.x; ++b) t += partials[(long long)b * NTOT + tid];
        totals[tid] = t;
    }
}

// ---- one generation of the genetic loop -------------------------------------------------------------------------------------------
// candidate kg = max(k * v, 2.0) in fp64 (v == nullptr: kg = k, the fitness of the starting anchors, committed unconditionally); fitness = mean of
// best [best > thr] over the points with kg rounded to fp32; the reducer commits k = kg, f = fg when fg > f (strict) and notes it in *accepted
__global__ __launch_bounds__(BT) void anchor_evolve_kernel(const float* __restrict__ wh, long long N, double* __restrict__ k, double* __restrict__ f, int n,
                                                            const double* __restrict__ v, float thr, double* __restrict__ partials, unsigned* __restrict__ ticket,
                                                            int* __restrict__ accepted) {
    __shared__ double s_kg[2 * MAX_N];
    __shared__ float s_k[2 * MAX_N];
    __shared__ double s_red[BT];
    __shared__ int s_flag, s_take;
    const int tid = threadIdx.x;
    if (tid < 2 * n) {
        const double kg = v ? fmax(k[tid] * v[tid], 2.0) : k[tid];
        s_kg[tid] = kg;
        s_k[tid] = (float)kg;
    }
    __syncthreads();
    double acc = 0.0;
    for (long long i = (long long)blockIdx.x * BT + tid; i < N; i += (long long)gridDim.x * BT) {
        const float w = wh[2 * i], h = wh[2 * i + 1];
        float best = 0.0f;
        for (int j = 0; j < n; ++j) {
            const float x = ratio_metric(w, h, s_k[2 * j], s_k[2 * j + 1]);
            best = j == 0 ? x : fmaxf(best, x);
        }
        if (best > thr) acc += (double)best;
    }
    const double t = block_sum(acc, s_red);
    if (tid == 0) partials[blockIdx.x] = t;
    if (!last_block(ticket, gridDim.x, &s_flag)) return;   // every block has read k before its ticket: the reducer may overwrite it
    if (tid == 0) {
        double sum = 0.0;
        for (unsigned b = 0; b < gridDim.x; ++b) sum += partials[b];
        const double fg = sum / (double)N;
        const int take = !v || fg > *f;
        if (take) *f = fg;
        if (accepted) *accepted = take;
        s_take = take;
    }
    __syncthreads();
    if (s_take && v && tid < 2 * n) k[tid] = s_kg[tid];
}

// ---- one Lloyd iteration of R restarts ----------------------------------------------------------------------------------------------
// grid (blocks over the points, restart).  A chunk of BT points: every thread assigns its point to the nearest live code (squared distance, ties to the lowest
// index) and leaves (code, distance) in LDS; thread j < n then adds the chunk's members of code j in point order, thread n the distances.  The restart's last
// block adds the block partials in index order, writes the new means and the mean distance and drops a live code that got no member.
__global__ __launch_bounds__(BT) void kmeans_step_kernel(const float* __restrict__ pts, long long N, int n, double* __restrict__ codes, int* __restrict__ live,
                                                          unsigned long long frozen, double* __restrict__ dist, double* __restrict__ partials, unsigned* __restrict__ tickets) {
    __shared__ double s_c[2 * MAX_N];
    __shared__ int s_live[MAX_N];
    __shared__ int s_code[BT];
    __shared__ float s_px[BT], s_py[BT];
    __shared__ double s_d[BT];
    __shared__ int s_flag;
    const int r = blockIdx.y, tid = threadIdx.x;
    if ((frozen >> r) & 1ull) return;   // (uniform over the restart's blocks: its ticket stays untouched)
    double* cr = codes + (long long)r * 2 * n;
    int* lr = live + (long long)r * n;
    const int stride = 3 * n + 1;
    double* pr = partials + ((long long)r * gridDim.x + blockIdx.x) * stride;
    if (tid < 2 * n) s_c[tid] = cr[tid];
    if (tid < n) s_live[tid] = lr[tid];
    __syncthreads();
    double a0 = 0.0, a1 = 0.0, a2 = 0.0;   // thread j < n: sum x, sum y, members of code j; thread n: a0 = sum of the distances
    for (long long base = (long long)blockIdx.x * BT; base < N; base += (long long)gridDim.x * BT) {
        const long long i = base + tid;
        int c = -1;
        double bd = 0.0;
        if (i < N) {
            const float px = pts[2 * i], py = pts[2 * i + 1];
            for (int j = 0; j < n; ++j) {
                if (!s_live[j]) continue;
                const double dx = (double)px - s_c[2 * j], dy = (double)py - s_c[2 * j + 1];
                const double d2 = dx * dx + dy * dy;
                if (c < 0 || d2 < bd) { bd = d2; c = j; }
            }
            s_px[tid] = px;
            s_py[tid] = py;
        }
        s_code[tid] = c;
        s_d[tid] = sqrt(bd);
        __syncthreads();
        const int cnt = (int)(N - base < BT ? N - base : BT);
        if (tid < n) {
            for (int p = 0; p < cnt; ++p)
                if (s_code[p] == tid) {
                    a0 += (double)s_px[p];
                    a1 += (double)s_py[p];
                    a2 += 1.0;
                }
        } else if (tid == n) {
            for (int p = 0; p < cnt; ++p) a0 += s_d[p];
        }
        __syncthreads();
    }
    if (tid < n) {
        pr[3 * tid] = a0;
        pr[3 * tid + 1] = a1;
        pr[3 * tid + 2] = a2;
    } else if (tid == n) {
        pr[3 * n] = a0;
    }
    if (!last_block(tickets + r, gridDim.x, &s_flag)) return;
    const double* p0 = partials + (long long)r * gridDim.x * stride;
    if (tid < n) {
        double sx = 0.0, sy = 0.0, m = 0.0;
        for (unsigned b = 0; b < gridDim.x; ++b) {
            const double* p = p0 + (long long)b * stride + 3 * tid;
            sx += p[0];
            sy += p[1];
            m += p[2];
        }
        if (m > 0.0) {
            cr[2 * tid] = sx / m;
            cr[2 * tid + 1] = sy / m;
        } else {
            lr[tid] = 0;
        }
    } else if (tid == n) {
        double s = 0.0;
        for (unsigned b = 0; b < gridDim.x; ++b) s += p0[(long long)b * stride + 3 * n];
        dist[r] = s / (double)N;
    }
}

bool aligned8(const void* p) { return ((uintptr_t)p & 7) == 0; }

}  // namespace

extern "C" size_t y3_anchor_workspace_bytes(int64_t N, int32_t n, int32_t R) {
    if (N < 1 || N > 0x7fffffffLL || n < 1 || n > MAX_N || R < 0 || R > MAX_R) {
        y3_set_error("y3_anchor_workspace_bytes: bad geometry (N %lld, n %d in 1 .. %d, R %d in 0 .. %d)", (long long)N, n, MAX_N, R, MAX_R);
        return 0;
    }
    const size_t metric = (size_t)point_blocks(N, MAX_BLOCKS) * NTOT * sizeof(double);
    const size_t km = (size_t)R * (size_t)point_blocks(N, KM_BLOCKS) * (size_t)(3 * n + 1) * sizeof(double);
    return TICKET_BYTES + (metric > km ? metric : km);
}

extern "C" int y3_anchor_metrics(const float* wh, int64_t N, const double* k, int32_t n, float thr, double* totals, void* workspace, size_t workspace_bytes, void* stream) {
    if (!wh || !k || !totals || !workspace) Y3_FAIL("y3_anchor_metrics: null argument");
    if (n < 1 || n > MAX_N) Y3_FAIL("y3_anchor_metrics: %d anchors unsupported (1 .. %d)", n, MAX_N);
    if (N < 1 || N > 0x7fffffffLL) Y3_FAIL("y3_anchor_metrics: bad label count N %lld (1 .. 2^31 - 1)", (long long)N);
    if (!aligned8(k) || !aligned8(totals) || !aligned8(workspace)) Y3_FAIL("y3_anchor_metrics: fp64 buffers and the workspace must be 8-byte aligned");
    const size_t need = y3_anchor_workspace_bytes(N, n, 0);
    if (workspace_bytes < need) Y3_FAIL("y3_anchor_metrics: the workspace needs %zu bytes, %zu given", need, workspace_bytes);
    hipStream_t st = (hipStream_t)stream;
    Y3_HIP(hipMemsetAsync(workspace, 0, TICKET_BYTES, st));
    hipLaunchKernelGGL(anchor_metrics_kernel, dim3((unsigned)point_blocks(N, MAX_BLOCKS)), dim3(BT), 0, st, wh, (long long)N, k, n, thr,
                       (double*)((char*)workspace + TICKET_BYTES), (unsigned*)workspace, totals);
    Y3_CHECK_LAUNCH();
    return 0;
}

extern "C" int y3_anchor_evolve(const float* wh, int64_t N, double* k, double* f, int32_t n, const double* v, int32_t gen, float thr, int32_t* accepted, void* workspace,
                                size_t workspace_bytes, void* stream) {
    if (!wh || !k || !f || !workspace || (gen > 0 && (!v || !accepted))) Y3_FAIL("y3_anchor_evolve: null argument");
    if (n < 1 || n > MAX_N) Y3_FAIL("y3_anchor_evolve: %d anchors unsupported (1 .. %d)", n, MAX_N);
    if (N < 1 || N > 0x7fffffffLL) Y3_FAIL("y3_anchor_evolve: bad label count N %lld (1 .. 2^31 - 1)", (long long)N);
    if (gen < 0) Y3_FAIL("y3_anchor_evolve: gen %d is negative", gen);
    if (!aligned8(k) || !aligned8(f) || !aligned8(v) || !aligned8(workspace)) Y3_FAIL("y3_anchor_evolve: fp64 buffers and the workspace must be 8-byte aligned");
    const size_t need = y3_anchor_workspace_bytes(N, n, 0);
    if (workspace_bytes < need) Y3_FAIL("y3_anchor_evolve: the workspace needs %zu bytes, %zu given", need, workspace_bytes);
    hipStream_t st = (hipStream_t)stream;
    Y3_HIP(hipMemsetAsync(workspace, 0, TICKET_BYTES, st));
    const dim3 grid((unsigned)point_blocks(N, MAX_BLOCKS));
    double* partials = (double*)((char*)workspace + TICKET_BYTES);
    for (int g = -1; g < gen; ++g) {   // g == -1: the fitness of the starting anchors
        hipLaunchKernelGGL(anchor_evolve_kernel, grid, dim3(BT), 0, st, wh, (long long)N, k, f, n, g < 0 ? (const double*)nullptr : v + (size_t)g * 2 * n, thr, partials,
                           (unsigned*)workspace, g < 0 ? (int*)nullptr : accepted + g);
        Y3_CHECK_LAUNCH();
    }
    return 0;
}

extern "C" int y3_kmeans_step(const float* pts, int64_t N, int32_t n, int32_t R, double* codes, int32_t* live, uint64_t frozen, double* dist, void* workspace,
                              size_t workspace_bytes, void* stream) {
    if (!pts || !codes || !live || !dist || !workspace) Y3_FAIL("y3_kmeans_step: null argument");
    if (n < 1 || n > MAX_N) Y3_FAIL("y3_kmeans_step: %d codes unsupported (1 .. %d)", n, MAX_N);
    if (N < 1 || N > 0x7fffffffLL) Y3_FAIL("y3_kmeans_step: bad point count N %lld (1 .. 2^31 - 1)", (long long)N);
    if (R < 1 || R > MAX_R) Y3_FAIL("y3_kmeans_step: %d restarts unsupported (1 .. %d)", R, MAX_R);
    if (!aligned8(codes) || !aligned8(dist) || !aligned8(workspace)) Y3_FAIL("y3_kmeans_step: fp64 buffers and the workspace must be 8-byte aligned");
    const size_t need = y3_anchor_workspace_bytes(N, n, R);
    if (workspace_bytes < need) Y3_FAIL("y3_kmeans_step: the workspace needs %zu bytes, %zu given", need, workspace_bytes);
    hipStream_t st = (hipStream_t)stream;
    Y3_HIP(hipMemsetAsync(workspace, 0, TICKET_BYTES, st));
    hipLaunchKernelGGL(kmeans_step_kernel, dim3((unsigned)point_blocks(N, KM_BLOCKS), (unsigned)R), dim3(BT), 0, st, pts, (long long)N, n, codes, live,
                       (unsigned long long)frozen, dist, (double*)((char*)workspace + TICKET_BYTES), (unsigned*)workspace);
    Y3_CHECK_LAUNCH();
    return 0;
}
