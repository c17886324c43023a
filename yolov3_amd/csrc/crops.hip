// The second-stage classifier hook of the detect loop on gfx950: reference utils/general.py:827-859 (apply_classifier; its call at detect.py:202-203), for the whole
// batch in three launches that read the batched NMS output (bs, max_det, 6) + counts where it lies --
//   * xyxy2xywh, rectangle to square, `* 1.3 + 30`, xywh2xyxy, .long()                      -> classifier_boxes_kernel, one thread per detection, into a table of its own
//     (the reference's `d = d.clone()`); with square = 0, gain 1.02 and pad 10 it is the box of upstream save_one_box (Detections.crop);
//   * scale_boxes of that table                                                             -> y3_scale_boxes (val_edge.hip), the one definition of that arithmetic;
//   * im0[y1:y2, x1:x2], cv2.resize to (S, S), BGR -> RGB, HWC -> CHW, float32, / 255         -> crop_resize_kernel, one block per (crop, band of output rows);
//   * x[i][pred_cls1 == pred_cls2]                                                          -> keep_matching_kernel, one block per image.
// The images lie in the uint8 arena of dataset.hip with its 32-byte records (offset, h, w; the other fields are not read).  cv2 is an un-vendored dependency: the
// 8-bit INTER_LINEAR arithmetic is the restatement y3_resize_u8.h shares with letterbox_u8_kernel, here with every coordinate and coefficient relative to the cutout.
// Whatever the tables hold, no read leaves an image's offset .. offset + 3 h w range or the arena, and no write leaves the outputs: a crop whose cutout is empty,
// whose box lies outside its image, whose image's record does not lie inside the arena or which the prefix does not place is written as zeros and counted in the
// status word.  fp32 arithmetic in the reference's operation order (built with -ffp-contract=off).
#include "y3_common.h"
#include "y3_resize_u8.h"

namespace {

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

constexpr int BT = 256;
constexpr int WAVE = 64;
constexpr int PASS = BT / WAVE;   // output rows of one pass: a wave per row
constexpr int MAX_S = 1024;
constexpr int BAND = 16;          // output rows of one block: the S column triples are formed once per block

// d[:, :4] of the reference after `.long()`, one thread per detection.  Rows at and beyond the image's count are written as zeros and not read.
__global__ __launch_bounds__(BT) void classifier_boxes_kernel(const float* __restrict__ rows, long long img_stride, int row_stride, const int* __restrict__ counts, int bs, int max_rows,
                                                                float gain, float pad, int square, float* __restrict__ out) {
    const long long idx = (long long)blockIdx.x * BT + threadIdx.x;
    if (idx >= (long long)bs * max_rows) return;
    const int img = (int)(idx / max_rows), r = (int)(idx - (long long)img * max_rows);
    float* o = out + idx * 4;
    if (counts && r >= counts[img]) {
        o[0] = 0.0f; o[1] = 0.0f; o[2] = 0.0f; o[3] = 0.0f;
        return;
    }
    const float* b = rows + img * img_stride + (long long)r * row_stride;
    const float x1 = b[0], y1 = b[1], x2 = b[2], y2 = b[3];
    const float cx = (x1 + x2) / 2.0f, cy = (y1 + y2) / 2.0f;   // xyxy2xywh
    float w = x2 - x1, h = y2 - y1;
    if (square) {   // b[:, 2:].max(1): a NaN wins, as torch's max
        const float m = (w != w || w > h) ? w : h;
        w = m;
        h = m;
    }
    w = w * gain + pad;   // a product, then a sum: two roundings
    h = h * gain + pad;
    const float hw = w / 2.0f, hh = h / 2.0f;   // xywh2xyxy
    // .long() truncates towards zero; the result goes back into the fp32 columns
    o[0] = (float)(long long)(cx - hw);
    o[1] = (float)(long long)(cy - hh);
    o[2] = (float)(long long)(cx + hw);
    o[3] = (float)(long long)(cy + hh);
}

struct CropTables {
    const y3_dataset_image* images;
    long long n_images, arena_bytes;
    const float* boxes;          // (bs, max_rows, 4): the scaled, clipped table
    const int* counts;
    const long long* prefix;     // (bs): crop k of image i is tile prefix[i] + k
    int bs, max_rows;
    long long n_tiles;
};

struct Cutout {
    long long base;   // first byte of the cutout's pixel (0, 0) in the arena
    int W, cw, ch;    // the image's width (the row pitch in pixels), the cutout's size
};

// int(v) of a clipped coordinate: truncation; anything that is no coordinate of an image (a NaN, a value below 0 or beyond 2^31) becomes a value the tests below refuse
Y3_DEV int coord(float v) { return (int)fminf(fmaxf(v, -1.0f), 2147483520.0f); }

// The cutout of detection k of image img, or false: the image's record does not lie inside the arena, the box lies outside the image, the cutout is empty.
Y3_DEV bool cutout_of(const CropTables& a, int img, int k, Cutout& c) {
    if (img < 0 || img >= a.bs || img >= a.n_images || k < 0 || k >= a.max_rows || k >= a.counts[img]) return false;
    const y3_dataset_image r = a.images[img];
    if (r.h < 1 || r.w < 1 || r.offset < 0 || r.offset > a.arena_bytes || (long long)r.h * r.w > (a.arena_bytes - r.offset) / 3) return false;
    const float* b = a.boxes + ((long long)img * a.max_rows + k) * 4;
    const int x1 = coord(b[0]), y1 = coord(b[1]), x2 = coord(b[2]), y2 = coord(b[3]);
    if (x1 < 0 || y1 < 0 || x2 > r.w || y2 > r.h || x2 - x1 < 1 || y2 - y1 < 1) return false;
    c.base = r.offset + ((long long)y1 * r.w + x1) * 3;
    c.W = r.w;
    c.cw = x2 - x1;
    c.ch = y2 - y1;
    return true;
}

// The (image, detection) of tile t: the last image whose prefix is <= t.  A prefix that does not place the tile inside an image's count fails in cutout_of.
Y3_DEV void tile_of(const CropTables& a, long long t, int& img, int& k) {
    int lo = 0, hi = a.bs - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (a.prefix[mid] <= t) lo = mid;
        else hi = mid - 1;
    }
    const long long d = t - a.prefix[lo];
    img = lo;
    k = d >= 0 && d < a.max_rows ? (int)d : -1;
}

struct CropArgs {
    CropTables t;
    const unsigned char* arena;
    void* dst;   // (n_tiles, 3, S, S)
    int S, bands, col_bytes;   // bands: blocks per tile; col_bytes: LDS bytes of the column triples, a multiple of 16
    y3_divisor seg_div;        // by the 16-byte stores (VEC) or the elements of one output row
    int* status;
};

// One block: rows [band * BAND, +BAND) of one tile, all three planes.
//   1. thread 0 finds the tile's cutout (or that it has none: the block then writes zeros, and the tile's first block counts it);
//   2. the S column triples (sx, a0, a1) go into LDS, once per block;
//   3. per pass a wave takes one output row: the row pair and its coefficients once per row, the lanes consecutive output columns -- their taps lie in two source
//      rows of the cutout, 6 consecutive bytes per lane -- and the three values of a pixel, value / 255 from the 256-entry table of IEEE quotients rounded once to D,
//      land in the wave's three staged plane rows (plane c from source channel 2 - c);
//   4. the block stores the pass's rows from LDS: 16 bytes per lane (VEC: S % 8 == 0 and dst 16-byte aligned) or element by element, the same values.
template <typename D, bool VEC> __global__ __launch_bounds__(BT) void crop_resize_kernel(const CropArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ float lut[256];
    __shared__ Cutout s_cut;
    __shared__ int s_ok;
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = __builtin_amdgcn_readfirstlane(tid >> 6), S = a.S;
    int* s_sx = reinterpret_cast<int*>(smem);
    int* s_ab = s_sx + S;   // a0 | a1 << 16 (both in 0 .. 2048)
    D* stage = reinterpret_cast<D*>(smem + a.col_bytes);   // [PASS][3][S]
    const long long t = blockIdx.x / a.bands;
    const int band = (int)(blockIdx.x - t * a.bands);
    lut[tid] = (float)tid / 255.0f;
    if (tid == 0) {
        int img, k;
        Cutout c = {0, 0, 0, 0};
        tile_of(a.t, t, img, k);
        const bool ok = cutout_of(a.t, img, k, c);
        s_cut = c;
        s_ok = ok ? 1 : 0;
        if (!ok && band == 0) atomicAdd(a.status, 1);
    }
    __syncthreads();
    const bool ok = s_ok != 0;
    const Cutout c = s_cut;
    if (ok) {
        const double scale_x = 1.0 / ((double)S / (double)c.cw);   // as cv2 computes it
        for (int dx = tid; dx < S; dx += BT) {
            int sx, a0, a1;
            y3_resize_coef(dx, scale_x, c.cw, true, sx, a0, a1);
            s_sx[dx] = sx;
            s_ab[dx] = a0 | (a1 << 16);
        }
    }
    __syncthreads();
    const double scale_y = ok ? 1.0 / ((double)S / (double)c.ch) : 0.0;
    const int y0 = band * BAND, y_end = y0 + BAND < S ? y0 + BAND : S;
    D* dst = reinterpret_cast<D*>(a.dst) + t * 3 * S * S;
    for (int yb = y0; yb < y_end; yb += PASS) {
        const int y = yb + wave;
        if (y < y_end) {
            D* st = stage + wave * 3 * S;
            if (ok) {
                int sy, b0, b1;
                y3_resize_coef(y, scale_y, c.ch, false, sy, b0, b1);
                const int r0 = sy < 0 ? 0 : (sy > c.ch - 1 ? c.ch - 1 : sy), r1 = sy + 1 < 0 ? 0 : (sy + 1 > c.ch - 1 ? c.ch - 1 : sy + 1);
                const unsigned char* q0 = a.arena + c.base + (long long)r0 * c.W * 3;
                const unsigned char* q1 = a.arena + c.base + (long long)r1 * c.W * 3;
                for (int dx = lane; dx < S; dx += WAVE) {
                    const int sx = s_sx[dx], ab = s_ab[dx], a0 = ab & 0xffff, a1 = ab >> 16;
                    const int sx1 = sx + 1 < c.cw ? sx + 1 : sx;   // weight 0 whenever it would fall outside
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch) {
                        const int h0v = (int)q0[sx * 3 + ch] * a0 + (int)q0[sx1 * 3 + ch] * a1;
                        const int h1v = (int)q1[sx * 3 + ch] * a0 + (int)q1[sx1 * 3 + ch] * a1;
                        const int v = (((b0 * (h0v >> 4)) >> 16) + ((b1 * (h1v >> 4)) >> 16) + 2) >> 2;
                        st[(2 - ch) * S + dx] = from_f32<D>(lut[v < 0 ? 0 : (v > 255 ? 255 : v)]);
                    }
                }
            } else {
                for (int e = lane; e < 3 * S; e += WAVE) st[e] = from_f32<D>(0.0f);
            }
        }
        __syncthreads();
        const int nrows = y_end - yb < PASS ? y_end - yb : PASS;
        if constexpr (VEC) {
            const int segs = S * (int)sizeof(D) / 16, items = nrows * 3 * segs;
            for (int e = tid; e < items; e += BT) {
                const int rp = y3_fdiv(e, a.seg_div), x = e - rp * segs, w = rp / 3, pl = rp - w * 3;
                const u32x4 q = reinterpret_cast<const u32x4*>(stage + (w * 3 + pl) * S)[x];
                reinterpret_cast<u32x4*>(dst + ((long long)pl * S + yb + w) * S)[x] = q;
            }
        } else {
            const int items = nrows * 3 * S;
            for (int e = tid; e < items; e += BT) {
                const int rp = y3_fdiv(e, a.seg_div), x = e - rp * S, w = rp / 3, pl = rp - w * 3;
                dst[((long long)pl * S + yb + w) * S + x] = stage[(w * 3 + pl) * S + x];
            }
        }
        __syncthreads();
    }
}

struct KeepArgs {
    CropTables t;
    const float* rows;
    long long img_stride;
    int row_stride;
    const long long* classes;   // (n_tiles): the classifier's class per tile
    float* out;                 // (bs, max_rows, 6)
    int* out_counts;            // (bs)
};

// One block per image.  The block walks the image's rows 256 at a time: a lane decides whether its row stays -- (long) cls equals the class of its tile, and the
// tile is one crop_resize_kernel did not count in the status word --, a ballot and the waves' counts give every survivor its place behind the survivors before it.
// Rows at and beyond the new count are written as zeros.
__global__ __launch_bounds__(BT) void keep_matching_kernel(const KeepArgs a) {
    __shared__ int s_wave[PASS];
    const int img = blockIdx.x, tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid >> 6;
    int n = a.t.counts[img];
    n = n < 0 ? 0 : (n > a.t.max_rows ? a.t.max_rows : n);
    const long long first = a.t.prefix[img];
    const float* src = a.rows + img * a.img_stride;
    float* out = a.out + (long long)img * a.t.max_rows * 6;
    int running = 0;
    for (int base = 0; base < n; base += BT) {
        const int r = base + tid;
        bool keep = false;
        float v[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        if (r < n) {
            const float* row = src + (long long)r * a.row_stride;
#pragma unroll
            for (int e = 0; e < 6; ++e) v[e] = row[e];
            const long long t = first + r;
            Cutout c;
            if (first >= 0 && t < a.t.n_tiles && cutout_of(a.t, img, r, c) && fabsf(v[5]) < 9.0e18f) keep = (long long)v[5] == a.classes[t];   // `.long()`: truncation towards zero
        }
        const unsigned long long vote = __ballot(keep);
        if (lane == 0) s_wave[wave] = __popcll(vote);
        __syncthreads();
        int before = __popcll(vote & ((1ull << lane) - 1ull)), all = 0;
#pragma unroll
        for (int w = 0; w < PASS; ++w) {
            before += w < wave ? s_wave[w] : 0;
            all += s_wave[w];
        }
        if (keep) {
            float* o = out + (long long)(running + before) * 6;   // (running + before <= r: inside the image's rows)
#pragma unroll
            for (int e = 0; e < 6; ++e) o[e] = v[e];
        }
        running += all;
        __syncthreads();
    }
    for (long long e = (long long)running * 6 + tid; e < (long long)a.t.max_rows * 6; e += BT) out[e] = 0.0f;
    if (tid == 0) a.out_counts[img] = running;
}

bool aligned(const void* p, uintptr_t n) { return ((uintptr_t)p & (n - 1)) == 0; }

// the refusals the two exports over the tables share, in the order of the augment exports: null, geometry (the tables', then the export's own: S or the row stride), alignment
int check_tables(const char* fn, const CropTables& t, bool other_null, int S, int row_stride) {
    if (other_null || !t.images || !t.boxes || !t.counts || !t.prefix) Y3_FAIL("%s: null argument", fn);
    if (t.n_images < 1 || t.n_images > 0x7fffffffLL || t.bs < 1 || t.bs > t.n_images || t.max_rows < 1 || t.n_tiles < 0 || t.n_tiles > (long long)t.bs * t.max_rows || t.arena_bytes < 4 ||
        (t.arena_bytes & 3))
        Y3_FAIL("%s: bad geometry (%lld images in 1 .. 2^31 - 1, a batch of %d in 1 .. %lld images of %d >= 1 rows, %lld tiles, an arena of %lld bytes, a positive multiple of 4)", fn,
                t.n_images, t.bs, t.n_images, t.max_rows, t.n_tiles, t.arena_bytes);
    if (S < 1 || S > MAX_S) Y3_FAIL("%s: bad geometry (crops of %d x %d, 1 .. %d)", fn, S, S, MAX_S);
    if (row_stride < 6) Y3_FAIL("%s: bad geometry (row stride %d)", fn, row_stride);
    if (!aligned(t.images, 8) || !aligned(t.prefix, 8) || !aligned(t.boxes, 4) || !aligned(t.counts, 4))
        Y3_FAIL("%s: the record table and the prefix must be 8-byte, the boxes and the counts 4-byte aligned", fn);
    return 0;
}

template <typename D> void launch_crops(const CropArgs& a, bool vec, long long blocks, size_t lds, hipStream_t st) {
    if (vec) hipLaunchKernelGGL((crop_resize_kernel<D, true>), dim3((unsigned)blocks), dim3(BT), lds, st, a);
    else hipLaunchKernelGGL((crop_resize_kernel<D, false>), dim3((unsigned)blocks), dim3(BT), lds, st, a);
}

}  // namespace

extern "C" int y3_classifier_boxes(const float* rows, int64_t img_stride, int32_t row_stride, const int32_t* counts, int32_t bs, int32_t max_rows, float gain, float pad,
                                   int32_t square, float* boxes, void* stream) {
    if (!rows || !boxes) Y3_FAIL("y3_classifier_boxes: null argument");
    if (bs < 0 || max_rows < 0 || row_stride < 4) Y3_FAIL("y3_classifier_boxes: bad geometry (bs %d, rows %d, row stride %d)", bs, max_rows, row_stride);
    const long long total = (long long)bs * max_rows;
    if (total > 0x7fffffffLL * BT) Y3_FAIL("y3_classifier_boxes: batch too large");
    if (total == 0) return 0;
    hipLaunchKernelGGL(classifier_boxes_kernel, dim3((unsigned)((total + BT - 1) / BT)), dim3(BT), 0, (hipStream_t)stream, rows, (long long)img_stride, row_stride, counts, bs, max_rows, gain,
                       pad, square ? 1 : 0, boxes);
    Y3_CHECK_LAUNCH();
    return 0;
}

extern "C" int y3_crop_resize(const uint8_t* arena, int64_t arena_bytes, const y3_dataset_image* images, int64_t n_images, const float* boxes, const int32_t* counts,
                              const int64_t* prefix, int32_t bs, int32_t max_rows, void* dst, int32_t dst_dtype, int64_t n_tiles, int32_t S, int32_t* status, void* stream) {
    const char* fn = "y3_crop_resize";
    CropArgs a;
    a.t.images = images; a.t.n_images = n_images; a.t.arena_bytes = arena_bytes; a.t.boxes = boxes; a.t.counts = counts; a.t.prefix = (const long long*)prefix;
    a.t.bs = bs; a.t.max_rows = max_rows; a.t.n_tiles = n_tiles;
    if (check_tables(fn, a.t, !arena || !status || (n_tiles > 0 && !dst), S, 6)) return -1;
    const int bands = (S + BAND - 1) / BAND;
    if (n_tiles * bands > 0x7fffffffLL) Y3_FAIL("%s: %lld crops of %d x %d are too many", fn, (long long)n_tiles, S, S);
    if (!aligned(arena, 16) || !aligned(status, 4)) Y3_FAIL("%s: the arena must be 16-byte, the status word 4-byte aligned", fn);
    if (dst_dtype != Y3_F16 && dst_dtype != Y3_BF16 && dst_dtype != Y3_F32) Y3_FAIL("%s: unsupported output dtype %d (float16 / bfloat16 / float32)", fn, dst_dtype);
    const int esize = dst_dtype == Y3_F32 ? 4 : 2;
    if (!aligned(dst, esize)) Y3_FAIL("%s: the output must be aligned to its element size", fn);
    if (n_tiles == 0) return 0;
    const bool vec = S % 8 == 0 && aligned(dst, 16);
    a.arena = arena; a.dst = dst; a.S = S; a.bands = bands; a.status = status;
    a.col_bytes = (int)y3_round_up((size_t)S * 8, 16);
    a.seg_div = y3_make_divisor(vec ? S * esize / 16 : S);
    const size_t lds = (size_t)a.col_bytes + (size_t)PASS * 3 * S * esize;   // <= 8 KB + 48 KB
    const long long blocks = n_tiles * bands;
    hipStream_t st = (hipStream_t)stream;
    switch (dst_dtype) {
        case Y3_F16: launch_crops<f16_t>(a, vec, blocks, lds, st); break;
        case Y3_BF16: launch_crops<bf16_t>(a, vec, blocks, lds, st); break;
        default: launch_crops<float>(a, vec, blocks, lds, st); break;
    }
    Y3_CHECK_LAUNCH();
    return 0;
}

extern "C" int y3_keep_matching(const float* rows, int64_t img_stride, int32_t row_stride, const int32_t* counts, const int64_t* prefix, int32_t bs, int32_t max_rows,
                                const int64_t* classes, int64_t n_tiles, const float* boxes, const y3_dataset_image* images, int64_t n_images, int64_t arena_bytes, float* out,
                                int32_t* out_counts, void* stream) {
    const char* fn = "y3_keep_matching";
    KeepArgs a;
    a.t.images = images; a.t.n_images = n_images; a.t.arena_bytes = arena_bytes; a.t.boxes = boxes; a.t.counts = counts; a.t.prefix = (const long long*)prefix;
    a.t.bs = bs; a.t.max_rows = max_rows; a.t.n_tiles = n_tiles;
    if (check_tables(fn, a.t, !rows || !out || !out_counts || (n_tiles > 0 && !classes), 1, row_stride)) return -1;
    if (!aligned(classes, 8) || !aligned(rows, 4) || !aligned(out, 4) || !aligned(out_counts, 4)) Y3_FAIL("%s: the classes must be 8-byte, the rows and the counts 4-byte aligned", fn);
    a.rows = rows; a.img_stride = img_stride; a.row_stride = row_stride; a.classes = (const long long*)classes; a.out = out; a.out_counts = out_counts;
    hipLaunchKernelGGL(keep_matching_kernel, dim3((unsigned)bs), dim3(BT), 0, (hipStream_t)stream, a);
    Y3_CHECK_LAUNCH();
    return 0;
}
