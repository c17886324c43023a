// A cached dataset kept in device memory, batched without a host loader (gfx950): what the reference's LoadImagesAndLabels.__getitem__ (utils/dataloaders.py:659-735) and
// collate_fn (:825-830) do per image on the host for an augment=False set whose images are cached already resized (`--cache ram`) --
//   * letterbox(auto=False, scaleup=False) in its pad-only branch (r == 1, utils/augmentations.py:104-134): a constant 114 border of (top, left) computed by the host;
//   * img.transpose((2, 0, 1))[::-1]: HWC -> CHW, BGR -> RGB;
//   * torch.stack of the batch                                                            -> dataset_batch_kernel, ONE launch per batch, uint8 or already divided by 255;
//   * xywhn2xyxy(labels, ratio w, ratio h, padw, padh), xyxy2xywhn(w=W, h=H, clip=True, eps=1e-3), the image column of collate_fn and torch.cat
//                                                                                         -> dataset_targets_kernel.
// The images lie back to back in one uint8 arena (16-byte aligned starts, 64-bit offsets) with one record per image; the labels in one fp32 (total, 5) table with n + 1 offsets.
// Every read is bounded by the arena / the table whatever the records and the indices hold: an image or a row that does not lie inside them is written as border / skipped.
// The label arithmetic is fp32 in the operation order of the two upstream functions (built with -ffp-contract=off; `/` is the IEEE division NumPy performs).
#include "y3_common.h"

namespace {

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

constexpr int BT = 256;
constexpr int WAVE = 64;
constexpr int STAGE_DW = 4096;    // LDS dwords of the staged source rows (16 KB)
constexpr int MAX_ROWS = 64;      // output rows of one block
constexpr int MAX_W = 4096;
constexpr int BORDER = 114;
constexpr int TG_MAX_BS = 1024;   // images of one batch (the prefix of their label counts lives in LDS)

struct BatchArgs {
    const unsigned char* arena;
    long long arena_bytes;
    const y3_dataset_image* images;
    long long n_images;
    const long long* indices;
    long long first;
    void* dst;
    int count, H, W, rows, pitch_dw, segs, total_rows;   // rows: output rows per block; pitch_dw: LDS dwords per staged row; segs: 16-byte stores per output row
    y3_divisor seg_div;
};

// the image behind slot b of the batch, or -1
Y3_DEV long long image_of(const long long* indices, long long first, long long n_images, int b) {
    const long long img = indices ? indices[b] : first + b;
    return img >= 0 && img < n_images ? img : -1;
}

template <typename D> Y3_DEV void store_px(D* d, const float* v);   // 16 bytes: 16 / sizeof(D) values
template <> Y3_DEV void store_px<float>(float* d, const float* v) {
    const f32x4 q = {v[0], v[1], v[2], v[3]};
    *reinterpret_cast<f32x4*>(d) = q;
}
template <> Y3_DEV void store_px<f16_t>(f16_t* d, const float* v) {
    const u32x4 q = {pack2<f16_t>(v[0], v[1]), pack2<f16_t>(v[2], v[3]), pack2<f16_t>(v[4], v[5]), pack2<f16_t>(v[6], v[7])};
    *reinterpret_cast<u32x4*>(d) = q;
}
template <> Y3_DEV void store_px<bf16_t>(bf16_t* d, const float* v) {
    const u32x4 q = {pack2<bf16_t>(v[0], v[1]), pack2<bf16_t>(v[2], v[3]), pack2<bf16_t>(v[4], v[5]), pack2<bf16_t>(v[6], v[7])};
    *reinterpret_cast<u32x4*>(d) = q;
}

// One block: `rows` consecutive rows of the (count * H) output rows of the batch, all three channel planes of each.
//   1. one thread per row reads the image's record: the source row (3 w interleaved bytes, in general not 4-byte aligned) or "all border";
//   2. a wave per row copies the dwords that cover the source row into LDS, coalesced, from the 4-byte aligned address below it (the arena is 16-byte aligned and a
//      multiple of 4 bytes long, so the covering dwords lie inside it);
//   3. every lane takes PX = 16 / sizeof(D) consecutive output pixels of one row: it reads the 3 PX source bytes (+ the shift) as dwords from LDS, shifts them into
//      place with v_alignbyte, picks byte 2 - c of every pixel for plane c and stores 16 bytes per plane.  Pixels outside the image are BORDER; a floating output takes
//      value / 255 from a 256-entry table -- the IEEE quotient `im.to(dtype) / 255` rounds from (every uint8 is exact in fp16 / bf16, torch divides in fp32 and rounds once).
template <typename D> __global__ __launch_bounds__(BT) void dataset_batch_kernel(const BatchArgs a) {
    constexpr bool U8 = sizeof(D) == 1;
    constexpr int PX = 16 / (int)sizeof(D), NA = 3 * PX / 4;   // pixels of a lane, aligned source dwords of a lane
    __shared__ unsigned stage[STAGE_DW];
    __shared__ float lut[U8 ? 1 : 256];
    __shared__ long long s_src[MAX_ROWS], s_dst[MAX_ROWS];   // first covering dword of the source row in the arena; first element of the output row in plane 0
    __shared__ int s_ndw[MAX_ROWS], s_shift[MAX_ROWS], s_left[MAX_ROWS], s_w[MAX_ROWS];   // s_ndw 0: the whole row is border
    const int tid = threadIdx.x;
    if constexpr (!U8) lut[tid] = (float)tid / 255.0f;
    if (tid < a.rows) {
        const int g = blockIdx.x * a.rows + tid;
        int ndw = 0, shift = 0, left = 0, w = 0;
        long long src = 0, dst = 0;
        if (g < a.total_rows) {
            const int b = g / a.H, y = g - b * a.H;
            dst = ((long long)b * 3 * a.H + y) * a.W;
            const long long img = image_of(a.indices, a.first, a.n_images, b);
            if (img >= 0) {
                const y3_dataset_image r = a.images[img];
                const int sy = y - r.top;
                if (r.w >= 1 && r.w <= a.W && r.h >= 1 && r.left >= 0 && r.left <= a.W - r.w && sy >= 0 && sy < r.h && r.offset >= 0) {
                    const long long row = r.offset + (long long)sy * 3 * r.w;   // (h, w <= 2^31 - 1: no overflow below 2^63 for any record that passes the next test)
                    if (row + 3LL * r.w <= a.arena_bytes) {
                        shift = (int)(row & 3);
                        src = row >> 2;
                        ndw = (shift + 3 * r.w + 3) >> 2;   // <= 3 W / 4 + 2 <= pitch_dw
                        left = r.left;
                        w = r.w;
                    }
                }
            }
        }
        s_src[tid] = src; s_dst[tid] = dst; s_ndw[tid] = ndw; s_shift[tid] = shift; s_left[tid] = left; s_w[tid] = w;
    }
    __syncthreads();
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & (WAVE - 1);
    const unsigned* g32 = reinterpret_cast<const unsigned*>(a.arena);
    for (int i = wave; i < a.rows; i += BT / WAVE) {
        const int ndw = s_ndw[i];
        const unsigned* s = g32 + s_src[i];
        unsigned* d = stage + i * a.pitch_dw;
        for (int j = lane; j < ndw; j += WAVE) d[j] = s[j];
    }
    __syncthreads();
    D* dst = (D*)a.dst;
    const long long plane = (long long)a.H * a.W;
    const int items = a.rows * a.segs;
    for (int it = tid; it < items; it += BT) {
        const int i = y3_fdiv(it, a.seg_div), x0 = (it - i * a.segs) * PX;
        if (blockIdx.x * a.rows + i >= a.total_rows) break;   // (rows ascend with it)
        const int ndw = s_ndw[i], left = s_left[i], w = s_w[i];
        unsigned al[NA];
        if (ndw) {
            const int bo = 3 * (x0 - left) + s_shift[i], base = bo >> 2;
            const unsigned sh = (unsigned)bo & 3u;
            const unsigned* row = stage + i * a.pitch_dw;
            unsigned q[NA + 1];
#pragma unroll
            for (int k = 0; k <= NA; ++k) q[k] = row[min(max(base + k, 0), a.pitch_dw - 1)];   // (a clamped dword only feeds pixels outside the image)
#pragma unroll
            for (int k = 0; k < NA; ++k) al[k] = __builtin_amdgcn_alignbyte(q[k + 1], q[k], sh);
        } else {
#pragma unroll
            for (int k = 0; k < NA; ++k) al[k] = 0;
        }
        unsigned char px[3][PX];   // [plane][pixel]
#pragma unroll
        for (int p = 0; p < PX; ++p) {
            const bool in = ndw && (unsigned)(x0 + p - left) < (unsigned)w;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int n = 3 * p + 2 - c;
                px[c][p] = in ? (unsigned char)((al[n >> 2] >> (8 * (n & 3))) & 0xffu) : (unsigned char)BORDER;
            }
        }
        D* d = dst + s_dst[i] + x0;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if constexpr (U8) {
                u32x4 o;
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    o[j] = (unsigned)px[c][4 * j] | ((unsigned)px[c][4 * j + 1] << 8) | ((unsigned)px[c][4 * j + 2] << 16) | ((unsigned)px[c][4 * j + 3] << 24);
                *reinterpret_cast<u32x4*>(d + c * plane) = o;
            } else {
                float v[PX];
#pragma unroll
                for (int p = 0; p < PX; ++p) v[p] = lut[px[c][p]];
                store_px<D>(d + c * plane, v);
            }
        }
    }
}

struct TargetArgs {
    const float* labels;
    const long long* label_offsets;
    const y3_dataset_image* images;
    long long n_images;
    const long long* indices;
    long long first;
    float* out;
    long long n_rows;
    long long* out_offsets;
    int count, H, W;
    float clip_w, clip_h;   // W - eps, H - eps: computed in double, rounded to fp32 once
};

// Every block forms the prefix of the batch's label counts in LDS (count <= TG_MAX_BS); a thread converts one row, found by bisection of the prefix.  Rows at or past the
// prefix's total (a caller whose n_rows is too large) are zeroed; rows past n_rows are not written.
__global__ __launch_bounds__(BT) void dataset_targets_kernel(const TargetArgs a) {
    __shared__ long long s_beg[TG_MAX_BS], s_pref[TG_MAX_BS + 1];
    __shared__ int s_img_w[TG_MAX_BS], s_img_h[TG_MAX_BS];
    const int tid = threadIdx.x;
    const long long total = a.label_offsets[a.n_images];
    for (int b = tid; b < a.count; b += BT) {
        const long long img = image_of(a.indices, a.first, a.n_images, b);
        long long beg = 0, end = 0;
        int w = 0, h = 0;
        if (img >= 0) {
            beg = a.label_offsets[img];
            end = a.label_offsets[img + 1];
            beg = beg < 0 ? 0 : (beg > total ? total : beg);   // a table that does not describe `labels` reads nothing outside it
            end = end < beg ? beg : (end > total ? total : end);
            w = a.images[img].w;
            h = a.images[img].h;
        }
        s_beg[b] = beg;
        s_pref[b + 1] = end - beg;
        s_img_w[b] = w;
        s_img_h[b] = h;
    }
    __syncthreads();
    if (tid == 0) {
        long long run = 0;
        s_pref[0] = 0;
        for (int b = 0; b < a.count; ++b) {
            run += s_pref[b + 1];
            s_pref[b + 1] = run;
        }
    }
    __syncthreads();
    if (blockIdx.x == 0)
        for (int b = tid; b <= a.count; b += BT) a.out_offsets[b] = s_pref[b] < a.n_rows ? s_pref[b] : a.n_rows;
    const long long have = s_pref[a.count];
    const float Wf = (float)a.W, Hf = (float)a.H;
    for (long long j = (long long)blockIdx.x * BT + tid; j < a.n_rows; j += (long long)gridDim.x * BT) {
        float* o = a.out + j * 6;
        if (j >= have) {
#pragma unroll
            for (int e = 0; e < 6; ++e) o[e] = 0.0f;
            continue;
        }
        int lo = 0, hi = a.count - 1;   // the last b with s_pref[b] <= j
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (s_pref[mid] <= j) lo = mid;
            else hi = mid - 1;
        }
        const float* l = a.labels + (s_beg[lo] + (j - s_pref[lo])) * 5;
        const float cls = l[0], xc = l[1], yc = l[2], bw = l[3], bh = l[4];
        const int w = s_img_w[lo], h = s_img_h[lo];
        const float wf = (float)w, hf = (float)h;                                           // ratio w, ratio h with ratio == 1
        const float padw = (float)(a.W - w) * 0.5f, padh = (float)(a.H - h) * 0.5f;         // letterbox's dw, dh: halves, exact
        // xywhn2xyxy
        const float hw2 = bw / 2.0f, hh2 = bh / 2.0f;
        float x1 = wf * (xc - hw2) + padw;
        float y1 = hf * (yc - hh2) + padh;
        float x2 = wf * (xc + hw2) + padw;
        float y2 = hf * (yc + hh2) + padh;
        // clip_boxes(x, (H - eps, W - eps)): minimum(maximum(v, 0), bound), a NaN stays
        x1 = x1 < 0.0f ? 0.0f : x1; x1 = x1 > a.clip_w ? a.clip_w : x1;
        x2 = x2 < 0.0f ? 0.0f : x2; x2 = x2 > a.clip_w ? a.clip_w : x2;
        y1 = y1 < 0.0f ? 0.0f : y1; y1 = y1 > a.clip_h ? a.clip_h : y1;
        y2 = y2 < 0.0f ? 0.0f : y2; y2 = y2 > a.clip_h ? a.clip_h : y2;
        // xyxy2xywhn
        o[0] = (float)lo;
        o[1] = cls;
        o[2] = ((x1 + x2) / 2.0f) / Wf;
        o[3] = ((y1 + y2) / 2.0f) / Hf;
        o[4] = (x2 - x1) / Wf;
        o[5] = (y2 - y1) / Hf;
    }
}

bool aligned(const void* p, uintptr_t n) { return ((uintptr_t)p & (n - 1)) == 0; }

// output rows per block: the count in 1 .. what LDS holds whose items fill the block's passes of BT lanes best (the larger count on a tie)
int rows_per_block(int pitch_dw, int segs, int total_rows) {
    int rmax = STAGE_DW / pitch_dw;
    if (rmax > MAX_ROWS) rmax = MAX_ROWS;
    if (rmax > total_rows) rmax = total_rows;
    int best = 1;
    double best_eff = 0.0;
    for (int r = 1; r <= rmax; ++r) {
        const long long items = (long long)r * segs, passes = (items + BT - 1) / BT;
        const double eff = (double)items / (double)(passes * BT);
        if (eff >= best_eff) { best_eff = eff; best = r; }
    }
    return best;
}

int check_set(const char* fn, const void* images, int64_t n_images, const void* indices, int64_t first, int32_t count, int32_t H, int32_t W) {
    if (!images) Y3_FAIL("%s: null argument", fn);
    if (n_images < 1 || n_images > 0x7fffffffLL || count < 0 || H < 1 || W < 1 || H > 0xffff || W > MAX_W)
        Y3_FAIL("%s: bad geometry (%lld images in 1 .. 2^31 - 1, a batch of %d x 3 x %d x %d, H <= 65535, W <= %d)", fn, (long long)n_images, count, H, W, MAX_W);
    if (W % 16) Y3_FAIL("%s: the batch width %d is not a multiple of 16", fn, W);
    if (!indices && (first < 0 || first + count > n_images)) Y3_FAIL("%s: images %lld .. %lld lie outside the %lld of the set", fn, (long long)first, (long long)first + count - 1, (long long)n_images);
    if (!aligned(images, 8) || !aligned(indices, 8)) Y3_FAIL("%s: the record table and the indices must be 8-byte aligned", fn);
    return 0;
}

}  // namespace

extern "C" int y3_dataset_batch(const uint8_t* arena, int64_t arena_bytes, const y3_dataset_image* images, int64_t n_images, const int64_t* indices, int64_t first, int32_t count,
                                void* dst, int32_t dst_dtype, int32_t H, int32_t W, void* stream) {
    if (!arena || !dst) Y3_FAIL("y3_dataset_batch: null argument");
    if (check_set("y3_dataset_batch", images, n_images, indices, first, count, H, W)) return -1;
    if (arena_bytes < 4 || (arena_bytes & 3)) Y3_FAIL("y3_dataset_batch: the arena's %lld bytes are not a positive multiple of 4", (long long)arena_bytes);
    if (!aligned(arena, 16) || !aligned(dst, 16)) Y3_FAIL("y3_dataset_batch: the arena and the output must be 16-byte aligned");
    if (dst_dtype != Y3_U8 && dst_dtype != Y3_F16 && dst_dtype != Y3_BF16 && dst_dtype != Y3_F32) Y3_FAIL("y3_dataset_batch: unsupported output dtype %d (uint8 / float16 / bfloat16 / float32)", dst_dtype);
    if ((long long)count * H > 0x7fffffffLL / 64) Y3_FAIL("y3_dataset_batch: a batch of %d x %d rows is too large", count, H);
    if (count == 0) return 0;
    const int esize = dst_dtype == Y3_U8 ? 1 : (dst_dtype == Y3_F32 ? 4 : 2);
    BatchArgs a;
    a.arena = arena; a.arena_bytes = arena_bytes; a.images = images; a.n_images = n_images; a.indices = (const long long*)indices; a.first = first; a.dst = dst;
    a.count = count; a.H = H; a.W = W; a.total_rows = count * H;
    a.pitch_dw = 3 * W / 4 + 4;
    a.segs = W * esize / 16;
    a.seg_div = y3_make_divisor(a.segs);
    a.rows = rows_per_block(a.pitch_dw, a.segs, a.total_rows);
    const dim3 grid((unsigned)((a.total_rows + a.rows - 1) / a.rows));
    hipStream_t st = (hipStream_t)stream;
    switch (dst_dtype) {
        case Y3_U8: hipLaunchKernelGGL(dataset_batch_kernel<unsigned char>, grid, dim3(BT), 0, st, a); break;
        case Y3_F16: hipLaunchKernelGGL(dataset_batch_kernel<f16_t>, grid, dim3(BT), 0, st, a); break;
        case Y3_BF16: hipLaunchKernelGGL(dataset_batch_kernel<bf16_t>, grid, dim3(BT), 0, st, a); break;
        default: hipLaunchKernelGGL(dataset_batch_kernel<float>, grid, dim3(BT), 0, st, a); break;
    }
    Y3_CHECK_LAUNCH();
    return 0;
}

extern "C" int y3_dataset_targets(const float* labels, const int64_t* label_offsets, const y3_dataset_image* images, int64_t n_images, const int64_t* indices, int64_t first,
                                  int32_t count, int32_t H, int32_t W, float* targets, int64_t n_rows, int64_t* offsets, void* stream) {
    if (!label_offsets || !offsets || (n_rows > 0 && (!labels || !targets))) Y3_FAIL("y3_dataset_targets: null argument");
    if (check_set("y3_dataset_targets", images, n_images, indices, first, count, H, W)) return -1;
    if (count > TG_MAX_BS) Y3_FAIL("y3_dataset_targets: a batch of %d images unsupported (0 .. %d)", count, TG_MAX_BS);
    if (n_rows < 0 || n_rows > 0x7fffffffLL / 6) Y3_FAIL("y3_dataset_targets: bad geometry (%lld rows)", (long long)n_rows);
    if (!aligned(label_offsets, 8) || !aligned(offsets, 8) || !aligned(labels, 4) || !aligned(targets, 4)) Y3_FAIL("y3_dataset_targets: the offsets must be 8-byte, the fp32 tables 4-byte aligned");
    TargetArgs a;
    a.labels = labels; a.label_offsets = (const long long*)label_offsets; a.images = images; a.n_images = n_images; a.indices = (const long long*)indices; a.first = first;
    a.out = targets; a.n_rows = n_rows; a.out_offsets = (long long*)offsets; a.count = count; a.H = H; a.W = W;
    a.clip_w = (float)((double)W - 1e-3);
    a.clip_h = (float)((double)H - 1e-3);
    long long blocks = (n_rows + BT - 1) / BT;
    if (blocks < 1) blocks = 1;   // no row: the offsets are still written
    if (blocks > 1024) blocks = 1024;
    hipLaunchKernelGGL(dataset_targets_kernel, dim3((unsigned)blocks), dim3(BT), 0, (hipStream_t)stream, a);
    Y3_CHECK_LAUNCH();
    return 0;
}
