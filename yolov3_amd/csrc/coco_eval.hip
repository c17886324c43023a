// COCO bbox evaluation of a predictions.json on gfx950: what reference val.py:464-477 hands to pycocotools' COCOeval after the run --
//   * COCOeval.computeIoU + evaluateImg (greedy matching per image, category, area range and IoU threshold, crowd / ignore handling) -> coco_match_kernel
//   * COCOeval.accumulate (precision at the recall samples, recall, the scores at those samples)                                         -> coco_accumulate_kernel
// All arithmetic is fp64 in pycocotools' operation order (built with -ffp-contract=off), counts are integers: the three result arrays equal pycocotools' bit for bit.
//
// Order.  A detection's image / category position is found by binary search in the sorted imgIds / catIds; one that is in neither list takes no part (it sorts
// behind everything).  Four stable LSD passes of rocPRIM's radix_sort_pairs over (key, row index):
//     image position, score descending (64-bit ordered key), category position   -> the ACCUMULATE order (category, score descending, image, arrival):
//                                                                                    np.argsort(-dtScores, kind="mergesort") over the concatenation in imgIds order
//     image position once more                                                   -> the PAIR order (image, category, score descending, arrival): evaluateImg's
// so one 64-bit pass serves both orders.  The match kernel walks the pair order and writes its rows at their accumulate-order position.
//
// Match.  One block per non-empty (image, category) pair, thread p = a T + t runs the greedy pass of area range a and threshold t over the pair's first `cap`
// detections (cap = maxDets[-1]) in score order.  The IoU of a (detection, ground truth) pair is recomputed where it is needed: every lane of the block computes
// the same value in the same instruction, so a tile would save nothing, and there is no limit on the ground truths of a pair.  "Not ignored first, ignored last"
// is two sweeps over the pair's ground truths in file order; the stop rule of evaluateImg (a non-ignored match is not given up for an ignored ground truth) is
// "no second sweep after a match in the first".  The matched flags of a pass are bytes in the workspace (G per pass, written and read by that pass's thread only).
//
// Accumulate.  One block per (category, area range, maxDets, threshold): curves of val_stats.hip's kind -- a forward walk in chunks of 1024 rows (block scan of the
// true positives) finds, for every recall sample, the first row whose recall reaches it; a backward walk gives the reversed running maximum of the precision there.
#include "y3_common.h"

#include <rocprim/rocprim.hpp>

namespace {

constexpr int BT = 1024;     // threads of an accumulate block = rows per chunk
constexpr int MT = 128;      // threads of a match block: one per (area range, threshold) pass
constexpr int MAX_T = 16, MAX_A = 8, MAX_M = 8, MAX_R = 1024;
constexpr double SPACING1 = 2.220446049250313e-16;   // np.spacing(1)
constexpr int MATCH_MAX_BLOCKS = 1 << 20;

static_assert(MAX_T * MAX_A <= MT, "one thread per greedy pass");

// position of v in the ascending, duplicate-free ids[0 .. n), or -1
Y3_DEV int id_position(const long long* __restrict__ ids, int n, long long v) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (ids[mid] < v) lo = mid + 1;
        else hi = mid;
    }
    return lo < n && ids[lo] == v ? lo : -1;
}

// ---- order -------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void coco_positions_kernel(const long long* __restrict__ det_img, const long long* __restrict__ det_cat, long long nd,
                                                              const long long* __restrict__ img_ids, int n_img, const long long* __restrict__ cat_ids, int K,
                                                              unsigned* __restrict__ ip, unsigned* __restrict__ kp, unsigned* __restrict__ key, unsigned* __restrict__ idx) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= nd) return;
    int a = id_position(img_ids, n_img, det_img[i]), b = id_position(cat_ids, K, det_cat[i]);
    if (a < 0 || b < 0) { a = n_img; b = K; }   // takes no part: behind every image and every category
    ip[i] = (unsigned)a;
    kp[i] = (unsigned)b;
    key[i] = (unsigned)a;
    idx[i] = (unsigned)i;
}

// ascending keys = descending scores (-0.0 counts as 0.0, as it compares)
__global__ __launch_bounds__(256) void coco_score_keys_kernel(const double* __restrict__ score, const unsigned* __restrict__ idx, long long nd, unsigned long long* __restrict__ key) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= nd) return;
    const unsigned long long b = (unsigned long long)__double_as_longlong(score[idx[i]] + 0.0);
    const unsigned long long ord = (b >> 63) ? ~b : (b | 0x8000000000000000ull);
    key[i] = ~ord;
}

__global__ __launch_bounds__(256) void coco_gather_kernel(const unsigned* __restrict__ table, const unsigned* __restrict__ idx, long long nd, unsigned* __restrict__ key) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < nd) key[i] = table[idx[i]];
}

// rows in accumulate order: their scores, the categories' segments, and the (image position, own index) pairs of the last pass
__global__ __launch_bounds__(256) void coco_rows_kernel(const double* __restrict__ score, const unsigned* __restrict__ ip, const unsigned* __restrict__ acc,
                                                         const unsigned* __restrict__ cat_sorted, long long nd, int K, double* __restrict__ row_score,
                                                         int* __restrict__ cat_begin, int* __restrict__ cat_end, unsigned* __restrict__ key, unsigned* __restrict__ iota) {
    const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
    if (j >= nd) return;
    const unsigned src = acc[j];
    row_score[j] = score[src];
    key[j] = ip[src];
    iota[j] = (unsigned)j;
    const int c = (int)cat_sorted[j];
    if (c < K) {
        if (j == 0 || (int)cat_sorted[j - 1] != c) cat_begin[c] = (int)j;
        if (j == nd - 1 || (int)cat_sorted[j + 1] != c) cat_end[c] = (int)(j + 1);
    }
}

// pair key of every row in pair order (image position * K + category position; n_img * K for a row that takes no part) and the list of the pairs' first rows
__global__ __launch_bounds__(256) void coco_pairs_kernel(const unsigned* __restrict__ img_sorted, const unsigned* __restrict__ kp, const unsigned* __restrict__ acc,
                                                          const unsigned* __restrict__ pair, long long nd, int n_img, int K, long long* __restrict__ pk,
                                                          unsigned* __restrict__ heads, int* __restrict__ n_heads) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= nd) return;
    const long long none = (long long)n_img * K;
    auto key_of = [&](long long r) { return (int)img_sorted[r] >= n_img ? none : (long long)img_sorted[r] * K + (long long)kp[acc[pair[r]]]; };
    const long long k = key_of(i);
    pk[i] = k;
    if (k < none && (i == 0 || key_of(i - 1) != k)) heads[atomicAdd(n_heads, 1)] = (unsigned)i;
}

// ---- match -------------------------------------------------------------------------------------------------------------------------
// maskUtils.iou for boxes [x, y, w, h] (pycocotools common/maskApi.c bbIou)
Y3_DEV double box_iou(double dx, double dy, double dw, double dh, double darea, const double* __restrict__ g, bool crowd) {
    const double w = fmin(dw + dx, g[2] + g[0]) - fmax(dx, g[0]);
    if (w <= 0) return 0.0;
    const double h = fmin(dh + dy, g[3] + g[1]) - fmax(dy, g[1]);
    if (h <= 0) return 0.0;
    const double i = w * h;
    const double u = crowd ? darea : darea + g[2] * g[3] - i;
    return i / u;
}

__global__ __launch_bounds__(256) void coco_npig_kernel(const double* __restrict__ gt_area, const unsigned char* __restrict__ gt_crowd, const int* __restrict__ gt_cat, long long ng,
                                                         int K, const double* __restrict__ area_rng, int A, int* __restrict__ npig) {
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    if (g >= ng) return;
    const int c = gt_cat[g];
    if (c < 0 || c >= K || gt_crowd[g]) return;
    const double ar = gt_area[g];
    for (int a = 0; a < A; ++a)
        if (!(ar < area_rng[2 * a] || ar > area_rng[2 * a + 1])) atomicAdd(npig + (long long)c * A + a, 1);
}

__global__ __launch_bounds__(MT) void coco_match_kernel(const long long* __restrict__ pk, const unsigned* __restrict__ heads, const int* __restrict__ n_heads, long long nd,
                                                         const unsigned* __restrict__ pair, const unsigned* __restrict__ acc, const double* __restrict__ det_box,
                                                         const double* __restrict__ gt_box, const double* __restrict__ gt_area, const unsigned char* __restrict__ gt_crowd,
                                                         const int* __restrict__ gt_off, long long ng, const double* __restrict__ iou_thrs, int T,
                                                         const double* __restrict__ area_rng, int A, int cap, unsigned char* gtm, int* __restrict__ row_rank,
                                                         unsigned short* __restrict__ row_match, unsigned short* __restrict__ row_ignore) {
    __shared__ unsigned char s_m[MT], s_i[MT];
    __shared__ long long s_end;
    const int tid = threadIdx.x, P = A * T;
    const bool active = tid < P;
    const int a = active ? tid / T : 0, t = active ? tid % T : 0;
    const double thr = fmin(iou_thrs[t], 1 - 1e-10), lo = area_rng[2 * a], hi = area_rng[2 * a + 1];
    const int pairs = *n_heads;
    for (int p = blockIdx.x; p < pairs; p += gridDim.x) {
        const long long start = heads[p];
        const long long key = pk[start];
        if (tid == 0) {   // the pair's rows end where the key changes (keys ascend)
            long long l = start + 1, h = nd;
            while (l < h) {
                const long long mid = l + ((h - l) >> 1);
                if (pk[mid] > key) h = mid;
                else l = mid + 1;
            }
            s_end = l;
        }
        __syncthreads();
        const long long n = s_end - start;
        const int D = (int)(n < cap ? n : cap);
        for (long long r = tid; r < n; r += MT) row_rank[pair[start + r]] = (int)r;
        long long g0 = gt_off[key], g1 = gt_off[key + 1];
        g0 = g0 < 0 ? 0 : (g0 > ng ? ng : g0);   // offsets that do not describe the table read nothing outside it
        g1 = g1 < g0 ? g0 : (g1 > ng ? ng : g1);
        const int G = (int)(g1 - g0);
        unsigned char* mine = gtm + g0 * P + (long long)tid * G;   // matched flags of this pass, one per ground truth of the pair
        for (int d = 0; d < D; ++d) {
            const unsigned j = pair[start + d];
            const double* db = det_box + 4ll * acc[j];
            const double dx = db[0], dy = db[1], dw = db[2], dh = db[3];
            const double darea = dw * dh;
            int m = -1;
            bool ig_m = false;
            if (active) {
                double iou = thr;
                for (int sweep = 0; sweep < 2 && m < 0; ++sweep) {   // not ignored first, ignored last; no second sweep after a match in the first (the stop rule)
                    for (int g = 0; g < G; ++g) {
                        const bool crowd = gt_crowd[g0 + g] != 0;
                        const double ar = gt_area[g0 + g];
                        const bool ig = crowd || ar < lo || ar > hi;
                        if (ig != (sweep == 1)) continue;
                        if (mine[g] && !crowd) continue;
                        const double v = box_iou(dx, dy, dw, dh, darea, gt_box + 4 * (g0 + g), crowd);
                        if (v < iou) continue;
                        iou = v;
                        m = g;
                        ig_m = ig;
                    }
                }
                if (m >= 0) mine[m] = 1;
            }
            s_m[tid] = m >= 0;
            s_i[tid] = m >= 0 ? ig_m : (darea < lo || darea > hi);
            __syncthreads();
            if (tid < A) {
                unsigned mm = 0, ii = 0;
                for (int q = 0; q < T; ++q) {
                    mm |= (unsigned)s_m[tid * T + q] << q;
                    ii |= (unsigned)s_i[tid * T + q] << q;
                }
                row_match[(long long)j * A + tid] = (unsigned short)mm;
                row_ignore[(long long)j * A + tid] = (unsigned short)ii;
            }
            __syncthreads();
        }
    }
}

// ---- block scans (Hillis-Steele over BT values in LDS, as val_stats.hip; the result of thread i lies in the returned array at [i]) ----------
Y3_DEV int* block_scan_add(int v, int* buf) {
    int *a = buf, *b = buf + BT;
    const int tid = threadIdx.x;
    __syncthreads();   // (the previous scan's result has been read)
    a[tid] = v;
    __syncthreads();
    for (int d = 1; d < BT; d <<= 1) {
        int x = a[tid];
        if (tid >= d) x += a[tid - d];
        b[tid] = x;
        __syncthreads();
        int* s = a; a = b; b = s;
    }
    return a;
}
Y3_DEV double* block_scan_max(double v, double* buf) {
    double *a = buf, *b = buf + BT;
    const int tid = threadIdx.x;
    __syncthreads();
    a[tid] = v;
    __syncthreads();
    for (int d = 1; d < BT; d <<= 1) {
        double x = a[tid];
        if (tid >= d) x = fmax(x, a[tid - d]);
        b[tid] = x;
        __syncthreads();
        double* s = a; a = b; b = s;
    }
    return a;
}

// ---- accumulate --------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void coco_fill_kernel(double* __restrict__ p, long long n, double v) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) p[i] = v;
}

// grid (K, A * M, T).  The rows of category k with rank < maxDets[m], in accumulate order, are the curve; a row is a true positive when it is matched and not ignored
// at (t, a), a false positive when it is neither.  rc = tp / npig, pr = tp / (fp + tp + spacing(1)), then the envelope and the searchsorted(rc, r, "left") samples.
__global__ __launch_bounds__(BT) void coco_accumulate_kernel(const double* __restrict__ row_score, const int* __restrict__ row_rank, const unsigned short* __restrict__ row_match,
                                                              const unsigned short* __restrict__ row_ignore, const int* __restrict__ cat_begin, const int* __restrict__ cat_end,
                                                              const int* __restrict__ npig, int K, int T, const double* __restrict__ rec_thrs, int R,
                                                              const int* __restrict__ max_dets, int M, int A, double* __restrict__ precision, double* __restrict__ scores,
                                                              double* __restrict__ recall) {
    __shared__ int s_int[2 * BT];
    __shared__ double s_dbl[2 * BT];
    __shared__ int s_tpc[BT];
    __shared__ long long s_target[MAX_R], s_row[MAX_R];
    __shared__ double s_env[MAX_R];
    __shared__ int s_first, s_fp;
    const int k = blockIdx.x, a = blockIdx.y / M, m = blockIdx.y % M, t = blockIdx.z, tid = threadIdx.x;
    const int np = npig[(long long)k * A + a];
    if (np <= 0) return;   // no ground truth to find: the cells stay -1
    const long long b = cat_begin[k], n = (long long)cat_end[k] - b;
    const int md = max_dets[m];
    const int* rk = row_rank + b;
    const unsigned short* mt = row_match + b * A + a;
    const unsigned short* ig = row_ignore + b * A + a;

    if (tid == 0) { s_first = 0x7fffffff; s_fp = 0; }
    if (tid < R) {   // c = the smallest true-positive count with c / npig >= r; the sample is the first row that reaches it (c == 0: the first row there is)
        const double x = rec_thrs[tid];
        long long c = (long long)ceil(x * (double)np);
        if (c < 0) c = 0;
        if (c > np) c = (long long)np + 1;
        while (c > 0 && (double)(c - 1) / (double)np >= x) --c;
        while (c <= np && (double)c / (double)np < x) ++c;
        s_target[tid] = c;
        s_row[tid] = -1;   // past the end
        s_env[tid] = 0.0;
    }
    __syncthreads();

    long long run = 0;
    for (long long base = 0; base < n; base += BT) {
        const long long i = base + tid;
        const bool keep = i < n && rk[i] < md;
        const bool hit = keep && ((mt[i * A] >> t) & 1), ign = keep && ((ig[i * A] >> t) & 1);
        const int h = hit && !ign, f = keep && !hit && !ign;
        const int* sc = block_scan_add(h, s_int);
        const int tot = sc[BT - 1];
        s_tpc[tid] = sc[tid];
        if (keep) atomicMin(&s_first, (int)i);
        const unsigned long long fb = __ballot(f);
        if ((tid & 63) == 0 && fb) atomicAdd(&s_fp, __popcll(fb));
        __syncthreads();
        if (tid < R) {
            const long long tg = s_target[tid];
            if (tg > run && tg <= run + tot) {
                int lo = 0, hi = BT - 1;   // first row of the chunk whose count reaches tg
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (run + s_tpc[mid] >= tg) hi = mid;
                    else lo = mid + 1;
                }
                s_row[tid] = base + lo;
            }
        }
        run += tot;
        __syncthreads();
    }
    const long long tp_total = run, fp_total = s_fp;
    if (tid < R && s_target[tid] == 0 && s_first != 0x7fffffff) s_row[tid] = s_first;
    __syncthreads();

    long long later_tp = 0, later_fp = 0;   // counts in the rows behind the chunk
    double carry = 0.0;                     // envelope behind the chunk (a precision is never negative)
    for (long long hi = n; hi > 0; hi -= BT) {
        const long long lo = hi > BT ? hi - BT : 0;
        const long long i = hi - 1 - tid;   // thread 0 takes the last row: a forward scan over the threads is a suffix scan over the rows
        const bool keep = i >= lo && rk[i] < md;
        const bool hit = keep && ((mt[i * A] >> t) & 1), ign = keep && ((ig[i * A] >> t) & 1);
        const int h = hit && !ign, f = keep && !hit && !ign;
        const int* sc = block_scan_add(h, s_int);
        const int tot_tp = sc[BT - 1];
        const long long tpc = tp_total - later_tp - sc[tid] + h;
        sc = block_scan_add(f, s_int);
        const int tot_fp = sc[BT - 1];
        const long long fpc = fp_total - later_fp - sc[tid] + f;
        const double tp = (double)tpc, fp = (double)fpc;
        const double pr = keep ? tp / (fp + tp + SPACING1) : -1.0;
        const double* sm = block_scan_max(pr, s_dbl);
        if (tid < R) {
            const long long row = s_row[tid];
            if (row >= lo && row < hi) s_env[tid] = fmax(sm[hi - 1 - row], carry);
        }
        carry = fmax(carry, sm[BT - 1]);
        later_tp += tot_tp;
        later_fp += tot_fp;
    }

    if (tid < R) {
        const long long row = s_row[tid];
        const long long o = ((((long long)t * R + tid) * K + k) * A + a) * M + m;
        precision[o] = row >= 0 ? s_env[tid] : 0.0;
        scores[o] = row >= 0 ? row_score[b + row] : 0.0;
    }
    if (tid == 0) recall[(((long long)t * K + k) * A + a) * M + m] = (double)tp_total / (double)np;   // rc[-1]; 0 without rows
}

// ---- workspace of y3_coco_match ---------------------------------------------------------------------------------------------------------
struct CocoWs {
    unsigned *ip, *kp, *k32a, *k32b, *idx_a, *idx_b, *pair, *heads;
    unsigned long long *k64a, *k64b;
    int* n_heads;
    unsigned char* gtm;
    void* tmp;
    size_t tmp_bytes, gtm_bytes, total;
};
unsigned bits_for(long long v) {   // bits that hold 0 .. v
    unsigned b = 1;
    while (b < 63 && (1ll << b) <= v) ++b;
    return b;
}
void coco_ws_layout(long long nd, long long ng, int T, int A, char* base, CocoWs& w) {
    size_t off = 0;
    auto take = [&](size_t bytes) {
        char* p = base ? base + off : nullptr;
        off += y3_round_up(bytes ? bytes : 1, 256);
        return p;
    };
    const size_t nn = (size_t)(nd > 0 ? nd : 1);
    w.ip = (unsigned*)take(nn * 4);
    w.kp = (unsigned*)take(nn * 4);
    w.k32a = (unsigned*)take(nn * 4);
    w.k32b = (unsigned*)take(nn * 4);
    w.idx_a = (unsigned*)take(nn * 4);
    w.idx_b = (unsigned*)take(nn * 4);
    w.pair = (unsigned*)take(nn * 4);
    w.heads = (unsigned*)take(nn * 4);
    w.k64a = (unsigned long long*)take(nn * 8);
    w.k64b = (unsigned long long*)take(nn * 8);
    w.n_heads = (int*)take(4);
    w.gtm_bytes = (size_t)(ng > 0 ? ng : 0) * (size_t)(T * A);
    w.gtm = (unsigned char*)take(w.gtm_bytes);
    size_t t32 = 0, t64 = 0;
    if (rocprim::radix_sort_pairs(nullptr, t32, (unsigned*)nullptr, (unsigned*)nullptr, (unsigned*)nullptr, (unsigned*)nullptr, nn, 0u, 32u, (hipStream_t)0) != hipSuccess ||
        rocprim::radix_sort_pairs(nullptr, t64, (unsigned long long*)nullptr, (unsigned long long*)nullptr, (unsigned*)nullptr, (unsigned*)nullptr, nn, 0u, 64u, (hipStream_t)0) != hipSuccess)
        t32 = t64 = nn * 24 + (1u << 20);   // no device to ask (a size query on a build machine): an upper estimate, two more copies of the pairs and the histograms
    w.tmp_bytes = t32 > t64 ? t32 : t64;
    w.tmp = take(w.tmp_bytes);
    w.total = off;
}

bool coco_dims_ok(int T, int A) { return T >= 1 && T <= MAX_T && A >= 1 && A <= MAX_A; }

}  // namespace

extern "C" size_t y3_coco_eval_workspace_bytes(int64_t n_det, int64_t n_gt, int32_t T, int32_t A) {
    if (n_det < 0 || n_det > 0x7fffffffLL || n_gt < 0 || n_gt > 0x7fffffffLL || !coco_dims_ok(T, A)) {
        y3_set_error("y3_coco_eval_workspace_bytes: bad geometry (%lld detections, %lld ground truths in 0 .. 2^31 - 1, T %d in 1 .. %d, A %d in 1 .. %d)", (long long)n_det,
                     (long long)n_gt, T, MAX_T, A, MAX_A);
        return 0;
    }
    CocoWs w;
    coco_ws_layout(n_det, n_gt, T, A, nullptr, w);
    return w.total;
}

extern "C" int y3_coco_match(const int64_t* det_img, const int64_t* det_cat, const double* det_box, const double* det_score, int64_t n_det, const int64_t* img_ids, int32_t n_img,
                             const int64_t* cat_ids, int32_t K, const double* gt_box, const double* gt_area, const uint8_t* gt_crowd, const int32_t* gt_cat, int64_t n_gt,
                             const int32_t* gt_offsets, const double* iou_thrs, int32_t T, const double* area_rng, int32_t A, int32_t max_det, double* row_score, int32_t* row_rank,
                             uint16_t* row_match, uint16_t* row_ignore, int32_t* cat_begin, int32_t* cat_end, int32_t* npig, void* workspace, size_t workspace_bytes, void* stream) {
    if (!img_ids || !cat_ids || !gt_offsets || !iou_thrs || !area_rng || !cat_begin || !cat_end || !npig || !workspace) Y3_FAIL("y3_coco_match: null argument");
    if (n_det < 0 || n_det > 0x7fffffffLL || n_gt < 0 || n_gt > 0x7fffffffLL) Y3_FAIL("y3_coco_match: bad counts (%lld detections, %lld ground truths in 0 .. 2^31 - 1)", (long long)n_det, (long long)n_gt);
    if (n_det > 0 && (!det_img || !det_cat || !det_box || !det_score || !row_score || !row_rank || !row_match || !row_ignore)) Y3_FAIL("y3_coco_match: null detections or rows");
    if (n_gt > 0 && (!gt_box || !gt_area || !gt_crowd || !gt_cat)) Y3_FAIL("y3_coco_match: null ground truth");
    if (n_img < 1 || K < 1 || (long long)n_img * K >= 0x7fffffffLL) Y3_FAIL("y3_coco_match: bad geometry (%d images, %d categories, their product below 2^31 - 1)", n_img, K);
    if (T < 1 || T > MAX_T) Y3_FAIL("y3_coco_match: %d IoU thresholds unsupported (1 .. %d: the matches of a row are one 16-bit mask)", T, MAX_T);
    if (A < 1 || A > MAX_A) Y3_FAIL("y3_coco_match: %d area ranges unsupported (1 .. %d)", A, MAX_A);
    if (max_det < 1) Y3_FAIL("y3_coco_match: max_det %d (the largest maxDets, at least 1)", max_det);
    if (((uintptr_t)workspace & 255) != 0) Y3_FAIL("y3_coco_match: the workspace must be 256-byte aligned");
    CocoWs w;
    coco_ws_layout(n_det, n_gt, T, A, (char*)workspace, w);
    if (workspace_bytes < w.total) Y3_FAIL("y3_coco_match: the workspace needs %zu bytes, %zu given", w.total, workspace_bytes);
    hipStream_t st = (hipStream_t)stream;
    Y3_HIP(hipMemsetAsync(npig, 0, (size_t)K * A * sizeof(int32_t), st));
    Y3_HIP(hipMemsetAsync(cat_begin, 0, (size_t)K * sizeof(int32_t), st));
    Y3_HIP(hipMemsetAsync(cat_end, 0, (size_t)K * sizeof(int32_t), st));
    if (n_gt > 0) {
        hipLaunchKernelGGL(coco_npig_kernel, dim3((unsigned)((n_gt + 255) / 256)), dim3(256), 0, st, gt_area, gt_crowd, gt_cat, (long long)n_gt, K, area_rng, A, npig);
        Y3_CHECK_LAUNCH();
    }
    if (n_det == 0) return 0;
    const long long nd = n_det;
    const unsigned blocks = (unsigned)((nd + 255) / 256);
    const unsigned img_bits = bits_for(n_img), cat_bits = bits_for(K);
    Y3_HIP(hipMemsetAsync(w.n_heads, 0, sizeof(int), st));
    if (w.gtm_bytes) Y3_HIP(hipMemsetAsync(w.gtm, 0, w.gtm_bytes, st));
    Y3_HIP(hipMemsetAsync(row_match, 0, (size_t)nd * A * sizeof(uint16_t), st));
    Y3_HIP(hipMemsetAsync(row_ignore, 0, (size_t)nd * A * sizeof(uint16_t), st));
    hipLaunchKernelGGL(coco_positions_kernel, dim3(blocks), dim3(256), 0, st, (const long long*)det_img, (const long long*)det_cat, nd, (const long long*)img_ids, n_img,
                       (const long long*)cat_ids, K, w.ip, w.kp, w.k32a, w.idx_a);
    Y3_CHECK_LAUNCH();
    size_t tb = w.tmp_bytes;
    if (rocprim::radix_sort_pairs(w.tmp, tb, w.k32a, w.k32b, w.idx_a, w.idx_b, (size_t)nd, 0u, img_bits, st) != hipSuccess) Y3_FAIL("y3_coco_match: sort by image failed");
    hipLaunchKernelGGL(coco_score_keys_kernel, dim3(blocks), dim3(256), 0, st, det_score, (const unsigned*)w.idx_b, nd, w.k64a);
    Y3_CHECK_LAUNCH();
    tb = w.tmp_bytes;
    if (rocprim::radix_sort_pairs(w.tmp, tb, w.k64a, w.k64b, w.idx_b, w.idx_a, (size_t)nd, 0u, 64u, st) != hipSuccess) Y3_FAIL("y3_coco_match: sort by score failed");
    hipLaunchKernelGGL(coco_gather_kernel, dim3(blocks), dim3(256), 0, st, (const unsigned*)w.kp, (const unsigned*)w.idx_a, nd, w.k32a);
    Y3_CHECK_LAUNCH();
    tb = w.tmp_bytes;
    if (rocprim::radix_sort_pairs(w.tmp, tb, w.k32a, w.k32b, w.idx_a, w.idx_b, (size_t)nd, 0u, cat_bits, st) != hipSuccess) Y3_FAIL("y3_coco_match: sort by category failed");
    // idx_b: the accumulate order; k32b: its category positions
    hipLaunchKernelGGL(coco_rows_kernel, dim3(blocks), dim3(256), 0, st, det_score, (const unsigned*)w.ip, (const unsigned*)w.idx_b, (const unsigned*)w.k32b, nd, K, row_score, cat_begin,
                       cat_end, w.k32a, w.idx_a);
    Y3_CHECK_LAUNCH();
    tb = w.tmp_bytes;
    if (rocprim::radix_sort_pairs(w.tmp, tb, w.k32a, w.k32b, w.idx_a, w.pair, (size_t)nd, 0u, img_bits, st) != hipSuccess) Y3_FAIL("y3_coco_match: sort into pairs failed");
    // pair[i]: accumulate-order position of the i-th row in pair order; k32b: its image position
    long long* pk = (long long*)w.k64a;
    hipLaunchKernelGGL(coco_pairs_kernel, dim3(blocks), dim3(256), 0, st, (const unsigned*)w.k32b, (const unsigned*)w.kp, (const unsigned*)w.idx_b, (const unsigned*)w.pair, nd, n_img, K, pk,
                       w.heads, w.n_heads);
    Y3_CHECK_LAUNCH();
    const unsigned mblocks = (unsigned)(nd < MATCH_MAX_BLOCKS ? nd : MATCH_MAX_BLOCKS);   // (at most one pair per row; a block walks the list with the grid's stride)
    hipLaunchKernelGGL(coco_match_kernel, dim3(mblocks), dim3(MT), 0, st, (const long long*)pk, (const unsigned*)w.heads, (const int*)w.n_heads, nd, (const unsigned*)w.pair,
                       (const unsigned*)w.idx_b, det_box, gt_box, gt_area, gt_crowd, gt_offsets, (long long)n_gt, iou_thrs, T, area_rng, A, max_det, w.gtm, row_rank,
                       (unsigned short*)row_match, (unsigned short*)row_ignore);
    Y3_CHECK_LAUNCH();
    return 0;
}

extern "C" int y3_coco_accumulate(const double* row_score, const int32_t* row_rank, const uint16_t* row_match, const uint16_t* row_ignore, int64_t n_det, const int32_t* cat_begin,
                                  const int32_t* cat_end, const int32_t* npig, int32_t K, int32_t T, const double* rec_thrs, int32_t R, const int32_t* max_dets, int32_t M, int32_t A,
                                  double* precision, double* scores, double* recall, void* stream) {
    if (!cat_begin || !cat_end || !npig || !rec_thrs || !max_dets || !precision || !scores || !recall) Y3_FAIL("y3_coco_accumulate: null argument");
    if (n_det < 0 || n_det > 0x7fffffffLL) Y3_FAIL("y3_coco_accumulate: bad count (%lld rows in 0 .. 2^31 - 1)", (long long)n_det);
    if (n_det > 0 && (!row_score || !row_rank || !row_match || !row_ignore)) Y3_FAIL("y3_coco_accumulate: null rows");
    if (K < 1) Y3_FAIL("y3_coco_accumulate: bad geometry (%d categories)", K);
    if (T < 1 || T > MAX_T) Y3_FAIL("y3_coco_accumulate: %d IoU thresholds unsupported (1 .. %d)", T, MAX_T);
    if (A < 1 || A > MAX_A) Y3_FAIL("y3_coco_accumulate: %d area ranges unsupported (1 .. %d)", A, MAX_A);
    if (M < 1 || M > MAX_M) Y3_FAIL("y3_coco_accumulate: %d maxDets unsupported (1 .. %d)", M, MAX_M);
    if (R < 1 || R > MAX_R) Y3_FAIL("y3_coco_accumulate: %d recall samples unsupported (1 .. %d)", R, MAX_R);
    hipStream_t st = (hipStream_t)stream;
    const long long cells = (long long)T * K * A * M;
    hipLaunchKernelGGL(coco_fill_kernel, dim3((unsigned)((cells * R + 255) / 256)), dim3(256), 0, st, precision, cells * R, -1.0);
    Y3_CHECK_LAUNCH();
    hipLaunchKernelGGL(coco_fill_kernel, dim3((unsigned)((cells * R + 255) / 256)), dim3(256), 0, st, scores, cells * R, -1.0);
    Y3_CHECK_LAUNCH();
    hipLaunchKernelGGL(coco_fill_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, st, recall, cells, -1.0);
    Y3_CHECK_LAUNCH();
    hipLaunchKernelGGL(coco_accumulate_kernel, dim3((unsigned)K, (unsigned)(A * M), (unsigned)T), dim3(BT), 0, st, row_score, row_rank, (const unsigned short*)row_match,
                       (const unsigned short*)row_ignore, cat_begin, cat_end, npig, K, T, rec_thrs, R, max_dets, M, A, precision, scores, recall);
    Y3_CHECK_LAUNCH();
    return 0;
}
