// Statistics of a validation run on gfx950: what reference val.py:386-428 does on the host after process_batch --
//   * stats.append(...) / torch.cat(...)                    -> val_stats_append_kernel / count_labels_kernel (dense device-resident rows, label histogram)
//   * ap_per_class + compute_ap (utils/metrics.py:22-120)    -> order (key build, rocPRIM radix sort, gather), curves_kernel, summary_kernel
//   * ConfusionMatrix.process_batch (utils/metrics.py:134-178, val.py:390,406) -> confusion_kernel, one block per image
//   * the label edge of val.py:371,401-403                    -> labels_native_kernel
// Curve arithmetic is fp64 in the reference's operation order (built with -ffp-contract=off), counts are integers.  Rows are ordered by (class ascending,
// confidence descending, arrival ascending): the last key is this library's documented tie rule (np.argsort(-conf, kind="stable") on the host).
// The global ordering is rocPRIM's radix_sort_pairs (stable LSD radix sort, the library links it for the NMS already); everything else is own kernels.
// np.interp is reproduced as the reference's NumPy runs it: for a sample x inside the table the LARGEST j with xp[j] <= x; fp[j] if x == xp[j] or j is the last
// index, else (fp[j+1] - fp[j]) / (xp[j+1] - xp[j]) * (x - xp[j]) + fp[j].  A recall curve that exceeds 1 (more hits than labels: synthetic statistics only) makes
// compute_ap's table [0, recall..., 1] non-monotone at its end; the one sample that can see it (x == 1) then follows NumPy's guessed bisection step by step.
#include "y3_common.h"

#include <rocprim/rocprim.hpp>

namespace {

constexpr int BT = 1024;        // threads of a curves block = rows per chunk
constexpr int NCONF = 1000;     // confidence grid of the P(conf) / R(conf) curves
constexpr int NREC = 101;       // COCO recall samples
constexpr int SMOOTH_WIN = 101; // upstream smooth(y, 0.1) on 1000 samples: round(1000 * 0.1 * 2) // 2 + 1
constexpr int OUT_HEAD = 4;     // out[0] classes present, out[1] chosen confidence index, out[2] any hit, out[3] labels counted
constexpr int CONF_CAP = 4096;  // detections per image of the confusion kernel (as y3_match_detections)

// ---- append ------------------------------------------------------------------------------------------------------------------
// blocks (image, 256 rows): an image's valid rows land behind the rows of the images before it (exclusive sum of the counts), behind dst_offset
__global__ __launch_bounds__(256) void val_stats_append_kernel(const float* __restrict__ conf, const float* __restrict__ cls, long long img_stride, int elem_stride,
                                                                 const int* __restrict__ counts, int max_det, const unsigned char* __restrict__ correct, int niou,
                                                                 float* __restrict__ dconf, int* __restrict__ dcls, unsigned short* __restrict__ dmask, long long dst_offset,
                                                                 long long capacity) {
    const int img = blockIdx.x;
    long long base = dst_offset;
    int n = max_det;
    if (counts) {
        for (int i = 0; i < img; ++i) base += min(max(counts[i], 0), max_det);
        n = min(max(counts[img], 0), max_det);
    } else {
        base += (long long)img * max_det;
    }
    const int r = blockIdx.y * 256 + threadIdx.x;
    if (r < n) {
        const long long o = base + r;
        if (o >= capacity) return;   // (the host sized the buffers from the same counts: never taken)
        const long long s = img * img_stride + (long long)r * elem_stride;
        const unsigned char* h = correct + ((long long)img * max_det + r) * niou;
        unsigned m = 0;
        for (int t = 0; t < niou; ++t) m |= (h[t] ? 1u : 0u) << t;
        dconf[o] = conf[s];
        dcls[o] = (int)cls[s];
        dmask[o] = (unsigned short)m;
    }
}

__global__ __launch_bounds__(256) void count_labels_kernel(const float* __restrict__ cls, int stride, long long n, int* __restrict__ nt, int nc) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int c = (int)cls[i * stride];
    if (c >= 0 && c < nc) atomicAdd(nt + c, 1);
}

// ---- order -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void stats_init_kernel(int* __restrict__ seg, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) seg[i] = 0;
}

// key = class (rows of a class outside [0, nc) go behind every class) : ~ordered(conf) -- ascending keys = class ascending, confidence descending
__global__ __launch_bounds__(256) void stats_keys_kernel(const float* __restrict__ conf, const int* __restrict__ cls, long long n, int nc, unsigned long long* __restrict__ keys,
                                                           unsigned* __restrict__ idx) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const unsigned b = __float_as_uint(conf[i]);
    const unsigned ord = (b & 0x80000000u) ? ~b : (b | 0x80000000u);   // ascending with the float
    const int c = cls[i];
    const unsigned cc = (c >= 0 && c < nc) ? (unsigned)c : (unsigned)nc;
    keys[i] = ((unsigned long long)cc << 32) | (unsigned long long)(~ord);
    idx[i] = (unsigned)i;
}

__global__ __launch_bounds__(256) void stats_gather_kernel(const unsigned long long* __restrict__ keys, const unsigned* __restrict__ idx, const float* __restrict__ conf,
                                                             const unsigned short* __restrict__ mask, long long n, int nc, float* __restrict__ sconf,
                                                             unsigned short* __restrict__ smask, int* __restrict__ seg_begin, int* __restrict__ seg_end, int* __restrict__ any_hit) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    unsigned short m = 0;
    if (i < n) {
        const unsigned src = idx[i];
        m = mask[src];
        sconf[i] = conf[src];
        smask[i] = m;
        const int c = (int)(keys[i] >> 32);
        if (c < nc) {
            if (i == 0 || (int)(keys[i - 1] >> 32) != c) seg_begin[c] = (int)i;
            if (i == n - 1 || (int)(keys[i + 1] >> 32) != c) seg_end[c] = (int)(i + 1);
        }
    }
    if (__ballot(m != 0) != 0 && (threadIdx.x & 63) == 0) atomicOr(any_hit, 1);
}

// ---- block scans (Hillis-Steele over BT values in LDS; the result of thread i lies in the returned array at [i]) ---------------------
Y3_DEV int* block_scan_add(int v, int* buf) {
    int *a = buf, *b = buf + BT;
    const int tid = threadIdx.x;
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

// NumPy's binary_search_with_guess (numpy/_core/src/multiarray/compiled_base.c) for key == 1 on compute_ap's table when the recall curve exceeds 1:
// "key < arr[i]" holds exactly for cnt < i <= n (arr[0 .. cnt] <= 1, the rows beyond are above 1, the closing sentinel arr[n + 1] is 1), len = n + 2.
Y3_DEV long long interp_search_key_one(long long cnt, long long n, long long guess) {
    const long long len = n + 2;
    auto less = [&](long long i) { return i > cnt && i <= n; };
    long long imin = 0, imax = len;
    if (len <= 4) {
        long long i = 1;
        for (; i < len && !less(i); ++i) {}
        return i - 1;
    }
    if (guess > len - 3) guess = len - 3;
    if (guess < 1) guess = 1;
    if (less(guess)) {
        if (less(guess - 1)) {
            imax = guess - 1;
            if (guess > 8 && !less(guess - 8)) imin = guess - 8;
        } else {
            return guess - 1;
        }
    } else {
        if (less(guess + 1)) return guess;
        if (less(guess + 2)) return guess + 1;
        imin = guess + 2;
        if (guess < len - 8 - 1 && less(guess + 8)) imax = guess + 8;
    }
    while (imin < imax) {
        const long long imid = imin + ((imax - imin) >> 1);
        if (!less(imid)) imin = imid + 1;
        else imax = imid;
    }
    return imin - 1;
}

// ---- curves ------------------------------------------------------------------------------------------------------------------
// One block per (class, threshold).  Forward walk over the class's segment in chunks of BT rows (block scan of the hits): the running TP count, from it the
// table index of every recall sample (the row of the (m + 1)-th hit, m the largest count with m / (n_l + eps) <= x) and, at threshold 0, the TP counts at the two
// rows around every confidence sample.  Backward walk: TP count and the reversed running maximum of the precision (compute_ap's envelope) at the sampled rows.
__global__ __launch_bounds__(BT) void curves_kernel(const float* __restrict__ sconf, const unsigned short* __restrict__ smask, const int* __restrict__ seg_begin,
                                                     const int* __restrict__ seg_end, const int* __restrict__ nt, int nc, int niou, double eps,
                                                     const double* __restrict__ cgrid, const double* __restrict__ rgrid, double* __restrict__ out,
                                                     double* __restrict__ pcurve, double* __restrict__ rcurve) {
    __shared__ int s_int[2 * BT];
    __shared__ double s_dbl[2 * BT];
    __shared__ int s_tpc[BT];
    __shared__ long long s_target[NREC], s_cnt[NREC], s_j[NREC];
    __shared__ int s_ta[NREC], s_tb[NREC];
    __shared__ double s_ea[NREC], s_eb[NREC], s_y[NREC];
    __shared__ int s_jq[NCONF], s_q0[NCONF], s_q1[NCONF];
    __shared__ int s_row;
    const int c = blockIdx.x, t = blockIdx.y, tid = threadIdx.x;
    const int nl = nt[c];
    if (nl <= 0) return;   // no labels: the class has no row in the result
    if (tid == 0) {
        int r = 0;
        for (int i = 0; i < c; ++i) r += nt[i] > 0;
        s_row = r;
    }
    __syncthreads();
    const int row = s_row;
    double* orow = out + OUT_HEAD + (long long)row * (niou + 6);
    const long long b = seg_begin[c], n = (long long)seg_end[c] - b;
    if (t == 0 && tid == 0) orow[0] = (double)c;
    if (n <= 0) {   // labels and no predictions: zeros (utils/metrics.py:56-57)
        if (tid == 0) orow[6 + t] = 0.0;
        if (t == 0)
            for (int q = tid; q < NCONF; q += BT) {
                pcurve[(long long)row * NCONF + q] = 0.0;
                rcurve[(long long)row * NCONF + q] = 0.0;
            }
        return;
    }
    const double den = (double)nl + eps;
    const float* cf = sconf + b;
    const unsigned short* mk = smask + b;

    if (tid < NREC) {
        const double x = rgrid[tid];
        long long m = (long long)floor(x * (double)nl);
        if (m < 0) m = 0;
        while ((double)(m + 1) / den <= x) ++m;
        while (m > 0 && (double)m / den > x) --m;
        s_target[tid] = m + 1;   // the hit that first pushes the recall above x
        s_cnt[tid] = n;          // rows with recall <= x (all of them until that hit is met)
    }
    if (t == 0) {
        for (int q = tid; q < NCONF; q += BT) {
            const double px = cgrid[q];
            long long lo = 0, hi = n;   // rows with conf >= px (conf descending)
            while (lo < hi) {
                const long long mid = lo + ((hi - lo) >> 1);
                if ((double)cf[mid] >= px) lo = mid + 1;
                else hi = mid;
            }
            s_jq[q] = (int)lo - 1;
            s_q0[q] = 0;
            s_q1[q] = 0;
        }
    }
    __syncthreads();

    long long run = 0;
    for (long long base = 0; base < n; base += BT) {
        const long long i = base + tid;
        const int h = i < n ? (mk[i] >> t) & 1 : 0;
        const int* sc = block_scan_add(h, s_int);
        const int tot = sc[BT - 1];
        s_tpc[tid] = (int)run + sc[tid];
        __syncthreads();
        if (tid < NREC) {
            const long long tg = s_target[tid];
            if (tg > run && tg <= run + tot) {
                int lo = 0, hi = BT - 1;   // first row of the chunk whose TP count reaches tg
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (s_tpc[mid] >= tg) hi = mid;
                    else lo = mid + 1;
                }
                s_cnt[tid] = base + lo;
            }
        }
        if (t == 0) {
            for (int q = tid; q < NCONF; q += BT) {
                const long long j = s_jq[q];
                if (j >= base && j < base + BT) s_q0[q] = s_tpc[j - base];
                if (j + 1 >= base && j + 1 < base + BT && j + 1 < n) s_q1[q] = s_tpc[j + 1 - base];
            }
        }
        run += tot;
        __syncthreads();
    }
    const long long tp_total = run;

    if (tid == 0) {   // table index of every recall sample, in sample order (the guess of NumPy's search is the previous sample's index)
        long long prev = 0;
        for (int k = 0; k < NREC; ++k) {
            const double x = rgrid[k];
            const long long cnt = s_cnt[k];
            long long j;
            if (cnt >= n) j = (x >= 1.0) ? n + 1 : n;
            else if (x < 1.0) j = cnt;
            else j = interp_search_key_one(cnt, n, prev);
            s_j[k] = j;
            prev = j;
        }
    }
    if (tid < NREC) {
        s_ta[tid] = 0; s_tb[tid] = 0;
        s_ea[tid] = 0.0; s_eb[tid] = 0.0;
    }
    __syncthreads();

    long long later = 0;     // hits in the rows behind the chunk
    double carry = 0.0;      // envelope behind the chunk (the closing sentinel: precision 0)
    for (long long hi = n; hi > 0; hi -= BT) {
        const long long lo = hi > BT ? hi - BT : 0;
        const long long i = hi - 1 - tid;   // thread 0 takes the last row: a forward scan over the threads is a suffix scan over the rows
        const bool valid = i >= lo;
        const int h = valid ? (mk[i] >> t) & 1 : 0;
        const int* sc = block_scan_add(h, s_int);
        const int tot = sc[BT - 1];
        const int tpc = (int)(tp_total - later) - sc[tid] + h;
        const double prec = valid ? (double)tpc / (double)(i + 1) : -1.0;
        const double* sm = block_scan_max(prec, s_dbl);
        s_tpc[tid] = tpc;
        __syncthreads();
        if (tid < NREC) {
            const long long ra = s_j[tid] - 1, rb = s_j[tid];   // table index j <-> row j - 1
            if (ra >= lo && ra < hi) { s_ta[tid] = s_tpc[hi - 1 - ra]; s_ea[tid] = fmax(sm[hi - 1 - ra], carry); }
            if (rb >= lo && rb < hi) { s_tb[tid] = s_tpc[hi - 1 - rb]; s_eb[tid] = fmax(sm[hi - 1 - rb], carry); }
        }
        const double chunk_max = sm[BT - 1];
        __syncthreads();
        carry = fmax(carry, chunk_max);
        later += tot;
    }

    if (tid < NREC) {
        const double x = rgrid[tid];
        const long long j = s_j[tid];
        // table entries j and j + 1: index 0 = (0, 1), index n + 1 = (1, 0), between them (recall, envelope) of row j - 1
        const double xa = j == 0 ? 0.0 : (j == n + 1 ? 1.0 : (double)s_ta[tid] / den);
        const double fa = j == 0 ? 1.0 : (j == n + 1 ? 0.0 : s_ea[tid]);
        double y;
        if (j == n + 1 || xa == x) {
            y = fa;
        } else {
            const double xb = j + 1 == n + 1 ? 1.0 : (double)s_tb[tid] / den;
            const double fb = j + 1 == n + 1 ? 0.0 : s_eb[tid];
            y = (fb - fa) / (xb - xa) * (x - xa) + fa;
        }
        s_y[tid] = y;
    }
    __syncthreads();
    if (tid == 0) {   // np.trapezoid: sum(d * (y[1:] + y[:-1]) / 2.0)
        double ap = 0.0;
        for (int k = 0; k + 1 < NREC; ++k) ap += (rgrid[k + 1] - rgrid[k]) * (s_y[k + 1] + s_y[k]) / 2.0;
        orow[6 + t] = ap;
    }
    if (t == 0) {
        for (int q = tid; q < NCONF; q += BT) {
            const long long j = s_jq[q];
            double r, p;
            if (j < 0) {   // left of the table
                r = 0.0;
                p = 1.0;
            } else {
                const double x = -cgrid[q], xa = -(double)cf[j];
                const double ra = (double)s_q0[q] / den, pa = (double)s_q0[q] / (double)(j + 1);
                if (j == n - 1 || xa == x) {
                    r = ra;
                    p = pa;
                } else {
                    const double xb = -(double)cf[j + 1];
                    const double rb = (double)s_q1[q] / den, pb = (double)s_q1[q] / (double)(j + 2);
                    r = (rb - ra) / (xb - xa) * (x - xa) + ra;
                    p = (pb - pa) / (xb - xa) * (x - xa) + pa;
                }
            }
            rcurve[(long long)row * NCONF + q] = r;
            pcurve[(long long)row * NCONF + q] = p;
        }
    }
}

// ---- summary -----------------------------------------------------------------------------------------------------------------
// F1 curves, their class mean, upstream smooth(., 0.1), the first arg-max, and P / R / F1 / tp / fp of every class at that confidence
__global__ __launch_bounds__(BT) void summary_kernel(const int* __restrict__ nt, int nc, int niou, double eps, const double* __restrict__ pcurve,
                                                      const double* __restrict__ rcurve, const int* __restrict__ any_hit, double* __restrict__ out) {
    __shared__ double s_yp[NCONF + SMOOTH_WIN - 1];
    __shared__ double s_val[BT];
    __shared__ int s_idx[BT];
    __shared__ int s_present;
    const int tid = threadIdx.x;
    if (tid == 0) {
        int r = 0;
        long long total = 0;
        for (int i = 0; i < nc; ++i) {
            r += nt[i] > 0;
            total += nt[i];
        }
        s_present = r;
        out[3] = (double)total;
    }
    __syncthreads();
    const int present = s_present;
    constexpr int HALF = SMOOTH_WIN / 2;
    if (tid < NCONF) {
        double acc = 0.0;
        for (int r = 0; r < present; ++r) {
            const double p = pcurve[(long long)r * NCONF + tid], rc = rcurve[(long long)r * NCONF + tid];
            acc += 2 * p * rc / (p + rc + eps);
        }
        const double mean = present > 0 ? acc / (double)present : 0.0;
        s_yp[HALF + tid] = mean;
        if (tid == 0)
            for (int i = 0; i < HALF; ++i) s_yp[i] = mean;
        if (tid == NCONF - 1)
            for (int i = 0; i < HALF; ++i) s_yp[HALF + NCONF + i] = mean;
    }
    __syncthreads();
    double v = -1.0;
    if (tid < NCONF) {
        const double w = 1.0 / (double)SMOOTH_WIN;
        v = 0.0;
        for (int i = 0; i < SMOOTH_WIN; ++i) v += s_yp[tid + i] * w;
    }
    s_val[tid] = v;
    s_idx[tid] = tid;
    __syncthreads();
    for (int d = BT / 2; d > 0; d >>= 1) {   // first maximum
        if (tid < d) {
            const double o = s_val[tid + d];
            const int oi = s_idx[tid + d];
            if (o > s_val[tid] || (o == s_val[tid] && oi < s_idx[tid])) { s_val[tid] = o; s_idx[tid] = oi; }
        }
        __syncthreads();
    }
    const int best = s_idx[0];
    if (tid == 0) {
        out[0] = (double)present;
        out[1] = (double)best;
        out[2] = (double)(*any_hit != 0);
    }
    for (int r = tid; r < present; r += BT) {
        double* orow = out + OUT_HEAD + (long long)r * (niou + 6);
        const int c = (int)orow[0];
        const double p = pcurve[(long long)r * NCONF + best], rc = rcurve[(long long)r * NCONF + best];
        const double f1 = 2 * p * rc / (p + rc + eps);
        const double tp = rint(rc * (double)nt[c]);
        const double fp = rint(tp / (p + eps) - tp);
        orow[1] = tp; orow[2] = fp; orow[3] = p; orow[4] = rc; orow[5] = f1;
    }
}

// ---- confusion matrix --------------------------------------------------------------------------------------------------------
Y3_DEV float pair_iou(const float* lb, const float* dt) {   // upstream box_iou(labels, detections)[l][d], eps = 1e-7 (as csrc/val_edge.hip)
    const float iw = fmaxf(fminf(lb[2], dt[2]) - fmaxf(lb[0], dt[0]), 0.0f);
    const float ih = fmaxf(fminf(lb[3], dt[3]) - fmaxf(lb[1], dt[1]), 0.0f);
    const float inter = iw * ih;
    const float a1 = (lb[2] - lb[0]) * (lb[3] - lb[1]), a2 = (dt[2] - dt[0]) * (dt[3] - dt[1]);
    return inter / (a1 + a2 - inter + 1e-7f);
}

Y3_DEV void cm_add(unsigned long long* matrix, int nc, int r, int c) {
    if (r >= 0 && r <= nc && c >= 0 && c <= nc) atomicAdd(matrix + (long long)r * (nc + 1) + c, 1ull);
}

// One block per image.  A detection above `conf` keeps its highest-IoU label over all classes (IoU > iou_thres); a label then keeps its highest-IoU detection
// among those.  Equal IoUs resolve to the lower index (the reference's argsort leaves them undefined).  class_only: `labels` holds the classes alone and the image
// has no detections (the `detections=None` form of val.py:390).
__global__ __launch_bounds__(256) void confusion_kernel(const float* __restrict__ dets, long long img_stride, int row_stride, const int* __restrict__ counts, int max_det,
                                                         const float* __restrict__ labels, int label_stride, const int* __restrict__ offs, int nc, float conf_thres,
                                                         float iou_thres, unsigned long long* __restrict__ matrix) {
    __shared__ int bl[CONF_CAP];
    __shared__ float biou[CONF_CAP];
    __shared__ unsigned char won[CONF_CAP];
    __shared__ int s_matches;
    const int img = blockIdx.x;
    int n = dets ? (counts ? counts[img] : max_det) : 0;
    n = min(max(n, 0), max_det);
    const int l0 = offs[img], l1 = offs[img + 1];
    if (l1 <= l0) return;   // no labels: val.py:400 never calls process_batch
    if (threadIdx.x == 0) s_matches = 0;
    const float* D = dets ? dets + img * img_stride : nullptr;
    for (int d = threadIdx.x; d < n; d += 256) {
        const float* dt = D + (long long)d * row_stride;
        int best = -1;
        float bv = -1.0f;
        if (dt[4] > conf_thres) {
            best = -2;   // kept, unmatched so far
            for (int l = l0; l < l1; ++l) {
                const float v = pair_iou(labels + (long long)l * label_stride + 1, dt);
                if (v > iou_thres && v > bv) { bv = v; best = l; }
            }
        }
        bl[d] = best;   // -1: below conf (does not exist for the matrix)
        biou[d] = bv;
        won[d] = 0;
    }
    __syncthreads();
    for (int l = l0 + threadIdx.x; l < l1; l += 256) {
        const int gc = (int)labels[(long long)l * label_stride];
        int win = -1;
        float wv = -1.0f;
        for (int d = 0; d < n; ++d)
            if (bl[d] == l && biou[d] > wv) { wv = biou[d]; win = d; }
        if (win >= 0) {
            won[win] = 1;
            atomicAdd(&s_matches, 1);
            cm_add(matrix, nc, (int)D[(long long)win * row_stride + 5], gc);
        } else {
            cm_add(matrix, nc, nc, gc);   // background FN
        }
    }
    __syncthreads();
    if (s_matches > 0)   // utils/metrics.py:175 `if n:` -- false positives are only counted for an image with a match
        for (int d = threadIdx.x; d < n; d += 256)
            if (bl[d] != -1 && !won[d]) cm_add(matrix, nc, (int)D[(long long)d * row_stride + 5], nc);
}

// ---- labels to native space ----------------------------------------------------------------------------------------------------
// val.py:371 (`targets[:, 2:] *= (w, h, w, h)`), :401 xywh2xyxy, :402 scale_boxes with the image's (gain, pad) and native shape; params[img] as y3_scale_boxes
__global__ __launch_bounds__(256) void labels_native_kernel(const float* __restrict__ targets, int nl, int bs, float width, float height, const float* __restrict__ params,
                                                             float* __restrict__ out, int* __restrict__ offs) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i <= bs) {   // labels are grouped by image (the collate function's order): offs[i] = first label of an image >= i
        int lo = 0, hi = nl;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if ((int)targets[(long long)mid * 6] < i) lo = mid + 1;
            else hi = mid;
        }
        offs[i] = lo;
    }
    if (i >= nl) return;
    const float* t = targets + (long long)i * 6;
    float* o = out + (long long)i * 5;
    const int img = (int)t[0];
    o[0] = t[1];
    const float x = t[2] * width, y = t[3] * height, hw = t[4] * width / 2, hh = t[5] * height / 2;
    float x1 = x - hw, y1 = y - hh, x2 = x + hw, y2 = y + hh;
    if (img >= 0 && img < bs) {
        const float gain = params[img * 5], px = params[img * 5 + 1], py = params[img * 5 + 2], w0 = params[img * 5 + 3], h0 = params[img * 5 + 4];
        x1 = fminf(fmaxf((x1 - px) / gain, 0.0f), w0);
        y1 = fminf(fmaxf((y1 - py) / gain, 0.0f), h0);
        x2 = fminf(fmaxf((x2 - px) / gain, 0.0f), w0);
        y2 = fminf(fmaxf((y2 - py) / gain, 0.0f), h0);
    }
    o[1] = x1; o[2] = y1; o[3] = x2; o[4] = y2;
}

// ---- workspace layout of y3_val_stats_compute -----------------------------------------------------------------------------------
struct StatsWs {
    unsigned long long *key_a, *key_b;
    unsigned *idx_a, *idx_b;
    float* sconf;
    unsigned short* smask;
    int *seg_begin, *seg_end, *any_hit;
    double *pcurve, *rcurve;
    void* tmp;
    size_t tmp_bytes, total;
};
int class_bits(int nc) {   // bits that hold 0 .. nc
    int b = 1;
    while ((1ll << b) <= nc) ++b;
    return b;
}
bool stats_ws_layout(long long n, int nc, char* base, StatsWs& w) {
    size_t off = 0;
    auto take = [&](size_t bytes) {
        char* p = base ? base + off : nullptr;
        off += y3_round_up(bytes, 256);
        return p;
    };
    const size_t nn = (size_t)(n > 0 ? n : 1);
    w.key_a = (unsigned long long*)take(nn * 8);
    w.key_b = (unsigned long long*)take(nn * 8);
    w.idx_a = (unsigned*)take(nn * 4);
    w.idx_b = (unsigned*)take(nn * 4);
    w.sconf = (float*)take(nn * 4);
    w.smask = (unsigned short*)take(nn * 2);
    w.seg_begin = (int*)take((size_t)(2 * nc + 1) * 4);   // seg_begin, seg_end, any_hit: one zeroing launch
    w.seg_end = w.seg_begin + nc;
    w.any_hit = w.seg_begin + 2 * nc;
    w.pcurve = (double*)take((size_t)nc * NCONF * 8);
    w.rcurve = (double*)take((size_t)nc * NCONF * 8);
    size_t tb = 0;
    if (rocprim::radix_sort_pairs(nullptr, tb, (unsigned long long*)nullptr, (unsigned long long*)nullptr, (unsigned*)nullptr, (unsigned*)nullptr, nn, 0u, (unsigned)(32 + class_bits(nc)),
                                  (hipStream_t)0) != hipSuccess)
        tb = nn * 16 + (1u << 20);   // no device to ask (a size query on a build machine): an upper estimate, two more copies of the pairs and the histograms
    w.tmp_bytes = tb;
    w.tmp = take(tb ? tb : 1);
    w.total = off;
    return true;
}

}  // namespace

extern "C" int y3_val_stats_append(const float* conf, const float* cls, int64_t img_stride, int32_t elem_stride, const int32_t* counts, int32_t bs, int32_t max_det,
                                   const uint8_t* correct, int32_t niou, float* dst_conf, int32_t* dst_cls, uint16_t* dst_mask, int64_t dst_offset, int64_t capacity, void* stream) {
    if (!conf || !cls || !correct || !dst_conf || !dst_cls || !dst_mask) Y3_FAIL("y3_val_stats_append: null argument");
    if (niou < 1 || niou > 16) Y3_FAIL("y3_val_stats_append: %d IoU thresholds unsupported (1 .. 16: the hits of a row are one 16-bit mask)", niou);
    if (bs < 0 || max_det < 0 || elem_stride < 1 || img_stride < 0) Y3_FAIL("y3_val_stats_append: bad geometry (bs %d, max_det %d, element stride %d)", bs, max_det, elem_stride);
    if (dst_offset < 0 || capacity < dst_offset) Y3_FAIL("y3_val_stats_append: offset %lld outside the capacity %lld", (long long)dst_offset, (long long)capacity);
    if (!counts && dst_offset + (int64_t)bs * max_det > capacity) Y3_FAIL("y3_val_stats_append: %lld rows do not fit the capacity %lld", (long long)bs * max_det, (long long)capacity);
    if (max_det > 65535 * 256) Y3_FAIL("y3_val_stats_append: %d rows per image unsupported (max %d)", max_det, 65535 * 256);
    if (bs == 0 || max_det == 0) return 0;
    hipLaunchKernelGGL(val_stats_append_kernel, dim3((unsigned)bs, (unsigned)((max_det + 255) / 256)), dim3(256), 0, (hipStream_t)stream, conf, cls, (long long)img_stride, elem_stride, counts, max_det, correct, niou,
                       dst_conf, dst_cls, (unsigned short*)dst_mask, (long long)dst_offset, (long long)capacity);
    Y3_CHECK_LAUNCH();
    return 0;
}

extern "C" int y3_val_stats_count_labels(const float* cls, int32_t stride, int64_t n, int32_t* nt, int32_t nc, void* stream) {
    if (!nt || (n > 0 && !cls)) Y3_FAIL("y3_val_stats_count_labels: null argument");
    if (n < 0 || stride < 1 || nc < 1) Y3_FAIL("y3_val_stats_count_labels: bad geometry (n %lld, stride %d, nc %d)", (long long)n, stride, nc);
    if (n == 0) return 0;
    hipLaunchKernelGGL(count_labels_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, cls, stride, (long long)n, nt, nc);
    Y3_CHECK_LAUNCH();
    return 0;
}

extern "C" size_t y3_val_stats_out_elems(int32_t nc, int32_t niou) {
    if (nc < 1 || niou < 1) return 0;
    return (size_t)OUT_HEAD + (size_t)nc * (size_t)(niou + 6);
}

extern "C" size_t y3_val_stats_workspace_bytes(int64_t n, int32_t nc) {
    if (n < 0 || n > 0x7fffffffLL || nc < 1) {
        y3_set_error("y3_val_stats_workspace_bytes: bad geometry (n %lld, nc %d)", (long long)n, nc);
        return 0;
    }
    StatsWs w;
    if (!stats_ws_layout(n, nc, nullptr, w)) {
        y3_set_error("y3_val_stats_workspace_bytes: rocPRIM size query failed");
        return 0;
    }
    return w.total;
}

extern "C" int y3_val_stats_compute(const float* conf, const int32_t* cls, const uint16_t* mask, int64_t n, const int32_t* nt, int32_t nc, int32_t niou, double eps,
                                    const double* conf_grid, const double* recall_grid, double* out, size_t out_elems, void* workspace, size_t workspace_bytes, void* stream) {
    if (!nt || !conf_grid || !recall_grid || !out || !workspace) Y3_FAIL("y3_val_stats_compute: null argument");
    if (n > 0 && (!conf || !cls || !mask)) Y3_FAIL("y3_val_stats_compute: null rows");
    if (n < 0 || n > 0x7fffffffLL || nc < 1) Y3_FAIL("y3_val_stats_compute: bad geometry (n %lld, nc %d)", (long long)n, nc);
    if (niou < 1 || niou > 16) Y3_FAIL("y3_val_stats_compute: %d IoU thresholds unsupported (1 .. 16)", niou);
    if (out_elems < y3_val_stats_out_elems(nc, niou)) Y3_FAIL("y3_val_stats_compute: the result needs %zu doubles, %zu given", y3_val_stats_out_elems(nc, niou), out_elems);
    if (((uintptr_t)workspace & 255) != 0) Y3_FAIL("y3_val_stats_compute: the workspace must be 256-byte aligned");
    StatsWs w;
    if (!stats_ws_layout(n, nc, (char*)workspace, w)) Y3_FAIL("y3_val_stats_compute: rocPRIM size query failed");
    if (workspace_bytes < w.total) Y3_FAIL("y3_val_stats_compute: the workspace needs %zu bytes, %zu given", w.total, workspace_bytes);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(stats_init_kernel, dim3((unsigned)((2 * nc + 1 + 255) / 256)), dim3(256), 0, st, w.seg_begin, 2 * nc + 1);
    Y3_CHECK_LAUNCH();
    if (n > 0) {
        const unsigned blocks = (unsigned)((n + 255) / 256);
        hipLaunchKernelGGL(stats_keys_kernel, dim3(blocks), dim3(256), 0, st, conf, cls, (long long)n, nc, w.key_a, w.idx_a);
        Y3_CHECK_LAUNCH();
        size_t tb = w.tmp_bytes;
        if (rocprim::radix_sort_pairs(w.tmp, tb, w.key_a, w.key_b, w.idx_a, w.idx_b, (size_t)n, 0u, (unsigned)(32 + class_bits(nc)), st) != hipSuccess)
            Y3_FAIL("y3_val_stats_compute: sort failed");
        hipLaunchKernelGGL(stats_gather_kernel, dim3(blocks), dim3(256), 0, st, w.key_b, w.idx_b, conf, (const unsigned short*)mask, (long long)n, nc, w.sconf, w.smask, w.seg_begin,
                           w.seg_end, w.any_hit);
        Y3_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(curves_kernel, dim3((unsigned)nc, (unsigned)niou), dim3(BT), 0, st, w.sconf, w.smask, w.seg_begin, w.seg_end, nt, nc, niou, eps, conf_grid, recall_grid, out,
                       w.pcurve, w.rcurve);
    Y3_CHECK_LAUNCH();
    hipLaunchKernelGGL(summary_kernel, dim3(1), dim3(BT), 0, st, nt, nc, niou, eps, w.pcurve, w.rcurve, w.any_hit, out);
    Y3_CHECK_LAUNCH();
    return 0;
}

extern "C" int y3_confusion_matrix(const float* dets, int64_t img_stride, int32_t row_stride, const int32_t* counts, int32_t bs, int32_t max_det, const float* labels,
                                   int32_t label_stride, const int32_t* label_offsets, int32_t nc, float conf_thres, float iou_thres, int64_t* matrix, void* stream) {
    if (!label_offsets || !matrix) Y3_FAIL("y3_confusion_matrix: null argument");
    if (bs < 0 || nc < 1) Y3_FAIL("y3_confusion_matrix: bad geometry (bs %d, nc %d)", bs, nc);
    if (max_det < 0 || max_det > CONF_CAP) Y3_FAIL("y3_confusion_matrix: max_det %d unsupported (max %d)", max_det, CONF_CAP);
    if (dets ? (row_stride < 6 || label_stride < 5) : (label_stride < 1 || max_det != 0))
        Y3_FAIL("y3_confusion_matrix: bad strides (rows %d, labels %d; without detections max_det must be 0)", row_stride, label_stride);
    if (bs == 0) return 0;
    hipLaunchKernelGGL(confusion_kernel, dim3((unsigned)bs), dim3(256), 0, (hipStream_t)stream, dets, (long long)img_stride, row_stride, counts, max_det, labels, label_stride,
                       label_offsets, nc, conf_thres, iou_thres, (unsigned long long*)matrix);
    Y3_CHECK_LAUNCH();
    return 0;
}

extern "C" int y3_labels_to_native(const float* targets, int32_t nl, int32_t bs, float width, float height, const float* params, float* labels_out, int32_t* offsets_out,
                                   void* stream) {
    if (!offsets_out || !params || (nl > 0 && (!targets || !labels_out))) Y3_FAIL("y3_labels_to_native: null argument");
    if (nl < 0 || bs < 0 || !(width > 0.0f) || !(height > 0.0f)) Y3_FAIL("y3_labels_to_native: bad geometry (nl %d, bs %d, %g x %g)", nl, bs, (double)width, (double)height);
    const int work = nl > bs + 1 ? nl : bs + 1;
    hipLaunchKernelGGL(labels_native_kernel, dim3((unsigned)((work + 255) / 256)), dim3(256), 0, (hipStream_t)stream, targets, nl, bs, width, height, params, labels_out, offsets_out);
    Y3_CHECK_LAUNCH();
    return 0;
}
