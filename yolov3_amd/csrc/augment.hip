// The train-mode loader on the device (gfx950): what the reference's LoadImagesAndLabels.__getitem__ does per item on the host for an augment=True set whose images are
// cached already resized (utils/dataloaders.py:659-735, 764-822; utils/augmentations.py:57-73, 137-216, 270-283) -- rect=False with its S x S items, and rect=True,
// whose items are letterboxed to their batch's H x W and take the letterbox branch only (the _hw exports; the square exports run the same kernels with H = W = S) --
//   * load_mosaic's paste of four images into a 2s x 2s canvas of 114 (or letterbox's border around one), random_perspective's cv2.warpAffine, mixup's blend, augment_hsv,
//     np.flipud / np.fliplr, transpose((2, 0, 1))[::-1] and torch.stack                      -> augment_batch_kernel, ONE launch per batch; the canvas is never materialised;
//   * xywhn2xyxy per tile, the clip to the canvas, the four-corner transform, box_candidates, xyxy2xywhn(clip=True, eps=1e-3), the flips of the labels, mixup's
//     concatenation and collate_fn                                                            -> augment_targets_kernel, ONE launch per batch;
//   * for a set with polygon labels, xyn2xy per tile, the clip, resample_segments, the transform of the 1000 points and segment2box per label row
//                                                                                             -> augment_polygons_kernel, ONE more launch ahead of the targets;
//   * for a batch of such a set in which some mosaic drew copy_paste candidates (utils/augmentations.py:219-240), the acceptance loop over bbox_ioa, the fill of
//     cv2.drawContours(FILLED) into im_new, the mirrored pixels, rows and polygons                -> copy_paste_select_kernel and copy_paste_raster_kernel ahead of the
//     CP forms of the three kernels above; every other batch launches the plain forms, which read no paste table.
// The host draws the random numbers and sends one y3_augment_item per item (yolov3_amd/augment.py); the images lie in the arena of csrc/dataset.hip with its record table.
// Every arena read is bounded by the arena whatever the records hold: a tile is cut down, when the block starts, to the part of its rectangle whose source pixels lie
// inside its image, and an image that does not lie inside the arena gives no tile at all (its pixels read as 114).
//
// The sampler is the 8-bit INTER_LINEAR of cv2.warpAffine as tests/augment_cases.py::warp_affine_u8 states it: the inverse matrix in float64 from the host, the source
// coordinate in 1 / 32 pixel as (rint((A01 y + A02) 1024) + 16 + rint(A00 x 1024)) >> 5, four taps weighted by (32 - fy | fy)(32 - fx | fx), + 512 >> 10; a tap outside the
// canvas or in no tile is 114.  The colour conversions are bgr2hsv_u8 (integer) and hsv2bgr_u8 (fp32, one rounding per operation) of the same file.  Built with
// -ffp-contract=off: every product and sum below rounds on its own, as NumPy's do.
#include "y3_common.h"

namespace {

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

constexpr int BT = 256;
constexpr int CHUNK = 1024;        // consecutive output pixels of one item per block (4 per lane)
constexpr int BORDER = 114;
constexpr int MAX_S = 4096;
constexpr int MAX_BS = 1024;
constexpr int SLOTS = 8;           // tiles of an item: 2 mosaics x 4

struct BatchArgs {
    const unsigned char* arena;
    long long arena_bytes;
    const y3_dataset_image* images;
    long long n_images;
    const y3_augment_item* items;
    void* dst;
    int count, H, W, pixels;       // pixels = H * W
    y3_divisor w_div;
};

struct BatchPasteArgs : BatchArgs { // what the copy-paste form of the sampler reads besides: the paste table of the batch (below) and the masks of its mosaics
    const int* paste;
    const unsigned* masks;
    int n_masks;
};

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

Y3_DEV int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// The tiles of one item as the block uses them: the rectangle on the canvas (empty when the tile is absent or invalid) and the arena address of canvas pixel (0, 0)
// of that tile's image: pixel (X, Y) of the rectangle is at base + Y * pitch + 3 X.
struct Tiles {
    int x1[SLOTS], y1[SLOTS], x2[SLOTS], y2[SLOTS], pitch[SLOTS];
    long long base[SLOTS];
};

Y3_DEV void setup_tile(Tiles& T, int slot, const BatchArgs& a, const y3_augment_item* it) {
    const int m = slot >> 2, t = slot & 3;
    int x1 = 0, y1 = 0, x2 = 0, y2 = 0, pitch = 0;
    long long base = 0;
    const y3_augment_mosaic* mo = &it->mosaics[m];
    if (m < clampi(it->nmos, 0, 2) && t < clampi(mo->ntiles, 0, 4)) {
        const y3_augment_tile tl = mo->tiles[t];
        const int canvas_w = clampi(mo->canvas, 0, 2 * MAX_S), canvas_h = mo->canvas_h ? clampi(mo->canvas_h, 0, 2 * MAX_S) : canvas_w;   // canvas_h 0: a square canvas
        if (tl.img >= 0 && tl.img < a.n_images) {
            const y3_dataset_image r = a.images[tl.img];
            if (r.w >= 1 && r.h >= 1 && r.w <= 0xffff && r.h <= 0xffff && r.offset >= 0 && r.offset <= a.arena_bytes && 3LL * r.w * r.h <= a.arena_bytes - r.offset) {
                // the part of the rectangle that lies on the canvas AND whose source pixel (X - padw, Y - padh) lies in the image
                const long long lx = tl.padw > 0 ? tl.padw : 0, ly = tl.padh > 0 ? tl.padh : 0;
                long long hx = (long long)tl.padw + r.w, hy = (long long)tl.padh + r.h;
                hx = hx < canvas_w ? hx : canvas_w;
                hy = hy < canvas_h ? hy : canvas_h;
                const long long ax1 = tl.x1 > lx ? tl.x1 : lx, ay1 = tl.y1 > ly ? tl.y1 : ly, ax2 = tl.x2 < hx ? tl.x2 : hx, ay2 = tl.y2 < hy ? tl.y2 : hy;
                if (ax1 < ax2 && ay1 < ay2) {
                    x1 = (int)ax1; y1 = (int)ay1; x2 = (int)ax2; y2 = (int)ay2;   // inside the canvas
                    pitch = 3 * r.w;
                    base = r.offset - ((long long)tl.padh * r.w + tl.padw) * 3;
                }
            }
        }
    }
    T.x1[slot] = x1; T.y1[slot] = y1; T.x2[slot] = x2; T.y2[slot] = y2; T.pitch[slot] = pitch; T.base[slot] = base;
}

// one tap of mosaic m: the canvas pixel (tx, ty) as B | G << 8 | R << 16.  CP (copy_paste's im[i] = flip(im)[i] with i = flip(im_new)): where bit (w - 1 - tx, ty) of the
// mosaic's mask is set the tap reads canvas pixel (w - 1 - tx, ty) instead, through the same tile lookup and the same 114.
template <bool CP> Y3_DEV unsigned tap(const Tiles& T, const unsigned char* arena, int m, long long tx, long long ty, const unsigned* mask, int w) {
    if constexpr (CP) {
        if (mask && tx >= 0 && tx < w && ty >= 0 && ty < w) {
            const long long fx = w - 1 - tx;
            if ((mask[ty * (w >> 5) + (fx >> 5)] >> (fx & 31)) & 1u) tx = fx;
        }
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int s = m * 4 + t;
        if (tx >= T.x1[s] && tx < T.x2[s] && ty >= T.y1[s] && ty < T.y2[s]) {
            const unsigned char* p = arena + (T.base[s] + ty * T.pitch[s] + tx * 3);
            return (unsigned)p[0] | ((unsigned)p[1] << 8) | ((unsigned)p[2] << 16);
        }
    }
    return (unsigned)BORDER * 0x010101u;
}

// the warped mosaic m at output pixel (x, y): warp_affine_u8
template <bool CP> Y3_DEV void sample(const Tiles& T, const unsigned char* arena, const y3_augment_mosaic* mo, int m, int x, int y, int* bgr, const unsigned* mask, int w) {
    const double a00 = mo->inv[0], a01 = mo->inv[1], a02 = mo->inv[2], a10 = mo->inv[3], a11 = mo->inv[4], a12 = mo->inv[5];
    const double xd = (double)x, yd = (double)y;
    const long long X = ((long long)rint((a01 * yd + a02) * 1024.0) + 16 + (long long)rint(a00 * xd * 1024.0)) >> 5;
    const long long Y = ((long long)rint((a11 * yd + a12) * 1024.0) + 16 + (long long)rint(a10 * xd * 1024.0)) >> 5;
    const long long sx = X >> 5, sy = Y >> 5;
    const int fx = (int)(X & 31), fy = (int)(Y & 31);
    const unsigned p00 = tap<CP>(T, arena, m, sx, sy, mask, w), p01 = tap<CP>(T, arena, m, sx + 1, sy, mask, w), p10 = tap<CP>(T, arena, m, sx, sy + 1, mask, w),
                   p11 = tap<CP>(T, arena, m, sx + 1, sy + 1, mask, w);
    const int w00 = (32 - fy) * (32 - fx), w01 = (32 - fy) * fx, w10 = fy * (32 - fx), w11 = fy * fx;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int sh = 8 * c;
        const int acc = w00 * (int)((p00 >> sh) & 255u) + w01 * (int)((p01 >> sh) & 255u) + w10 * (int)((p10 >> sh) & 255u) + w11 * (int)((p11 >> sh) & 255u);
        bgr[c] = (acc + 512) >> 10;
    }
}

// One block: CHUNK consecutive pixels (row-major) of one item.  Lane `tid` takes pixels tid, tid + 256, ...: consecutive lanes, consecutive pixels of a row, so with
// little rotation the taps of a wave lie next to each other in the arena.  The three bytes of a pixel go to LDS planes; then every lane stores 16 bytes per pass.
// A = BatchPasteArgs: the form launched for a batch in which some mosaic pastes; every other batch runs the plain form, which takes the arguments it always took.
template <typename D, typename A> __global__ __launch_bounds__(BT) void augment_batch_kernel(const A a) {
    constexpr bool CP = sizeof(A) != sizeof(BatchArgs);
    constexpr bool U8 = sizeof(D) == 1;
    constexpr int PX = 16 / (int)sizeof(D);
    __shared__ Tiles T;
    __shared__ unsigned char s_lut[3 * 256];
    __shared__ int s_sdiv[256], s_hdiv[256];
    __shared__ float s_q[U8 ? 1 : 256];
    __shared__ __attribute__((aligned(16))) unsigned char s_out[3][CHUNK];
    const int tid = threadIdx.x, b = blockIdx.y, first = blockIdx.x * CHUNK;
    const y3_augment_item* it = a.items + b;
    const int nmos = clampi(it->nmos, 0, 2);
    const bool hsv = it->hsv != 0, ud = it->flipud != 0, lr = it->fliplr != 0;
    if (tid < SLOTS) setup_tile(T, tid, a, it);
    if constexpr (!U8) s_q[tid] = (float)tid / 255.0f;
    if (hsv) {
        const unsigned char* l = &it->lut[0][0];
        for (int i = tid; i < 3 * 256; i += BT) s_lut[i] = l[i];
        s_sdiv[tid] = tid ? (int)rint((double)(255 << 12) / (1.0 * tid)) : 0;
        s_hdiv[tid] = tid ? (int)rint((double)(180 << 12) / (6.0 * tid)) : 0;
    }
    __syncthreads();
    const int valid = a.pixels - first < CHUNK ? a.pixels - first : CHUNK;   // a multiple of 256: H and W are multiples of 16
    const double r0 = it->ratio, r1 = it->ratio1;
    const unsigned* mask[2] = {nullptr, nullptr};
    const int cw = 2 * a.W;   // the canvas of a mosaic
    if constexpr (CP) {
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            const int mi = a.paste[2 * a.count + 1 + b * 2 + m];
            if (mi >= 0 && mi < a.n_masks && m < nmos && it->mosaics[m].clip && it->mosaics[m].canvas == cw) mask[m] = a.masks + (long long)mi * cw * (cw >> 5);
        }
    }
    for (int k = tid; k < valid; k += BT) {
        const int p = first + k;
        const int y = y3_fdiv(p, a.w_div), x = p - y * a.W;
        const int ox = lr ? a.W - 1 - x : x, oy = ud ? a.H - 1 - y : y;
        int c0[3] = {BORDER, BORDER, BORDER};
        if (nmos >= 1) sample<CP>(T, a.arena, &it->mosaics[0], 0, ox, oy, c0, mask[0], cw);
        if (nmos == 2) {   // mixup: (im * r + im2 * (1 - r)).astype(uint8) in float64
            int c1[3];
            sample<CP>(T, a.arena, &it->mosaics[1], 1, ox, oy, c1, mask[1], cw);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                double v = (double)c0[c] * r0 + (double)c1[c] * r1;
                v = v > 0.0 ? v : 0.0;   // (also a NaN of a record that is no record)
                v = v < 255.0 ? v : 255.0;
                c0[c] = (int)v;
            }
        }
        if (hsv) {
            // bgr2hsv_u8
            const int B = c0[0], G = c0[1], R = c0[2];
            const int v = max(max(B, G), R), diff = v - min(min(B, G), R);
            int s = (diff * s_sdiv[v] + (1 << 11)) >> 12;
            int h = v == R ? G - B : (v == G ? B - R + 2 * diff : R - G + 4 * diff);
            h = (h * s_hdiv[diff] + (1 << 11)) >> 12;
            h += h < 0 ? 180 : 0;
            h = clampi(h, 0, 255);
            s = clampi(s, 0, 255);
            // the look-up tables
            const int H2 = s_lut[h], S2 = s_lut[256 + s], V2 = s_lut[512 + v];
            // hsv2bgr_u8
            const float hf = (float)H2 * (6.0f / 180.0f), sf = (float)S2 * (1.0f / 255.0f), vf = (float)V2 * (1.0f / 255.0f);
            float sec = floorf(hf), f = hf - sec;
            int sector = (int)sec;
            if ((unsigned)sector >= 6u) { sector = 0; f = 0.0f; }
            const float t0 = vf, t1 = vf * (1.0f - sf), t2 = vf * (1.0f - sf * f), t3 = vf * (1.0f - sf * (1.0f - f));
            float fb, fg, fr;   // sector table {1,3,0} {1,0,2} {3,0,1} {0,2,1} {0,1,3} {2,1,0}
            switch (sector) {
                case 0: fb = t1; fg = t3; fr = t0; break;
                case 1: fb = t1; fg = t0; fr = t2; break;
                case 2: fb = t3; fg = t0; fr = t1; break;
                case 3: fb = t0; fg = t2; fr = t1; break;
                case 4: fb = t0; fg = t1; fr = t3; break;
                default: fb = t2; fg = t1; fr = t0; break;
            }
            if (S2 == 0) fb = fg = fr = vf;
            c0[0] = clampi((int)rintf(fb * 255.0f), 0, 255);
            c0[1] = clampi((int)rintf(fg * 255.0f), 0, 255);
            c0[2] = clampi((int)rintf(fr * 255.0f), 0, 255);
        }
        s_out[0][k] = (unsigned char)c0[2];   // RGB planes of a BGR pixel
        s_out[1][k] = (unsigned char)c0[1];
        s_out[2][k] = (unsigned char)c0[0];
    }
    __syncthreads();
    D* dst = (D*)a.dst + (long long)b * 3 * a.pixels + first;
    const int per = valid / PX, segs = 3 * per;   // 16-byte stores of the block
    for (int i = tid; i < segs; i += BT) {
        const int c = i / per, j = (i - c * per) * PX;
        if constexpr (U8) {
            *reinterpret_cast<u32x4*>(dst + (long long)c * a.pixels + j) = *reinterpret_cast<const u32x4*>(&s_out[c][j]);
        } else {
            float v[PX];
#pragma unroll
            for (int e = 0; e < PX; ++e) v[e] = s_q[s_out[c][j + e]];
            store_px<D>(dst + (long long)c * a.pixels + j, v);
        }
    }
}

struct TargetArgs {
    const float* labels;
    const long long* label_offsets;
    const y3_dataset_image* images;
    long long n_images;
    const y3_augment_item* items;
    float* out;
    long long n_rows;
    long long* out_offsets;
    int count, H, W;
    float clip_w, clip_h;   // W - eps, H - eps: computed in double, rounded to fp32 once
};

// the label rows of tile `slot` of the batch: [beg, end) of the table, or nothing
Y3_DEV void tile_rows(const TargetArgs& a, long long total, int slot, long long& beg, long long& end) {
    beg = end = 0;
    const y3_augment_item* it = a.items + (slot >> 3);
    const int m = (slot >> 2) & 1, t = slot & 3;
    const y3_augment_mosaic* mo = &it->mosaics[m];
    if (m >= clampi(it->nmos, 0, 2) || t >= clampi(mo->ntiles, 0, 4)) return;
    const long long img = mo->tiles[t].img;
    if (img < 0 || img >= a.n_images) return;
    beg = a.label_offsets[img];
    end = a.label_offsets[img + 1];
    beg = beg < 0 ? 0 : (beg > total ? total : beg);   // a table that does not describe `labels` reads nothing outside it
    end = end < beg ? beg : (end > total ? total : end);
    if (end - beg > (1 << 20)) end = beg + (1 << 20);
}

// xywhn2xyxy with the tile's w, h, lpadw, lpadh and load_mosaic's np.clip(x, 0, 2 s): label row `l` of the table as labels4 holds it (fp32; a rect item forms the
// product and the sum in fp64, below).  The one definition of the targets kernels and of copy-paste's selection.
Y3_DEV void canvas_box(const y3_augment_mosaic* mo, const y3_augment_tile& tl, const y3_dataset_image& im, const float* l, float& x1, float& y1, float& x2, float& y2) {
    const float xc = l[1], yc = l[2], bw = l[3], bh = l[4];
    const float wf = (float)im.w, hf = (float)im.h;
    const float hw2 = bw / 2.0f, hh2 = bh / 2.0f;
    if (tl.wide) {   // a rect item: letterbox took its shape from a NumPy array, so the ratio and the halves are float64 scalars: product and sum in fp64, one rounding
        x1 = (float)((double)wf * (double)(xc - hw2) + (double)tl.lpadw);
        y1 = (float)((double)hf * (double)(yc - hh2) + (double)tl.lpadh);
        x2 = (float)((double)wf * (double)(xc + hw2) + (double)tl.lpadw);
        y2 = (float)((double)hf * (double)(yc + hh2) + (double)tl.lpadh);
    } else {
        x1 = wf * (xc - hw2) + tl.lpadw;
        y1 = hf * (yc - hh2) + tl.lpadh;
        x2 = wf * (xc + hw2) + tl.lpadw;
        y2 = hf * (yc + hh2) + tl.lpadh;
    }
    if (mo->clip) {   // np.clip(x, 0, 2 s) of load_mosaic
        const float c = (float)mo->canvas, ch = mo->canvas_h ? (float)mo->canvas_h : c;
        x1 = x1 < 0.0f ? 0.0f : x1; x1 = x1 > c ? c : x1;
        y1 = y1 < 0.0f ? 0.0f : y1; y1 = y1 > ch ? ch : y1;
        x2 = x2 < 0.0f ? 0.0f : x2; x2 = x2 > c ? c : x2;
        y2 = y2 < 0.0f ? 0.0f : y2; y2 = y2 > ch ? ch : y2;
    }
}

// Copy-paste (reference utils/augmentations.py:219-240 inside load_mosaic).  The host draws js = random.sample(range(n), k) per mosaic and sends one int32 table per
// batch: 2 count + 1 offsets into js per (item, mosaic), then 2 count mask indices (-1: a mosaic without a paste), then the js of all mosaics back to back.  Every
// mosaic owns k positions directly after its tile rows in the position space of the polygon and targets kernels (counted with the rows of its fourth tile): slot e
// is candidate js[e], a dropped row unless the selection accepted it.  sel_i (nk, 4): accepted, j, the label-table row of polygon j, its tile; sel_f (nk, 5): the
// appended label row [cls, w - x2, y1, w - x1, y2].
struct PasteTables {
    const int* table;
    int nk;                 // the js of the batch
    int* sel_i;
    float* sel_f;
    unsigned* masks;        // (n_masks, 2 S, 2 S / 32): bit x & 31 of word (y, x >> 5) is im_new[y, x]
    int n_masks;
};

// the slots [beg, beg + k) of mosaic `mslot` in js, sel_i and sel_f; nothing where the table does not describe them
Y3_DEV void paste_range(const PasteTables& c, int mslot, int& beg, int& k) {
    beg = k = 0;
    if (!c.table) return;
    const int lo = clampi(c.table[mslot], 0, c.nk), hi = clampi(c.table[mslot + 1], lo, c.nk);
    beg = lo; k = hi - lo;
}

// Polygon labels (random_perspective's use_segments branch, utils/augmentations.py:183-194 with resample_segments and segment2box of utils/general.py): the vertex table
// of the set and what augment_polygons_kernel leaves per label position j of the batch for the polygon form of augment_targets_kernel.
struct PolyTables {
    const float* verts;              // (n_verts, 2) normalised
    const long long* vert_offsets;   // n_vert_rows + 1: row r of the label table owns vertices [vert_offsets[r], vert_offsets[r + 1])
    long long n_verts, n_vert_rows;
    double* boxes;                   // (ws_rows, 4) segment2box of the warped polygon, zeros when it has no point inside
    int* inside;                     // (ws_rows): 1 when that box was taken from points
    int* paths;                      // (count, 2) per item and mosaic: PATH_NONZERO | PATH_LACKS; the polygon path is taken when the word is PATH_NONZERO alone
    long long ws_rows;
};

constexpr int SAMPLES = 1000;        // resample_segments' n
constexpr int PATH_NONZERO = 1;      // some clipped coordinate of some polygon of the mosaic is not zero: any(x.any() for x in segments)
constexpr int PATH_LACKS = 2;        // some label row of the mosaic has no polygon: len(segments) != n

// vertex `idx` of the table on the canvas: xyn2xy(w, h, padw, padh) and np.clip(0, 2 s), both fp32; mirror: the vertex of a pasted polygon, fp32(2 s) - x
Y3_DEV void canvas_vertex(const float* verts, long long idx, float wf, float hf, float padw, float padh, float c, float& x, float& y, bool mirror = false) {
    x = wf * verts[2 * idx] + padw;
    y = hf * verts[2 * idx + 1] + padh;
    x = x < 0.0f ? 0.0f : x; x = x > c ? c : x;
    y = y < 0.0f ? 0.0f : y; y = y > c ? c : y;
    if (mirror) x = c - x;
}

// the vertices [vb, ve) of label-table row `row`; nothing where the offsets do not describe `verts`
Y3_DEV void row_vertices(const PolyTables& p, long long row, long long& vb, long long& ve) {
    vb = ve = 0;
    if (row < p.n_vert_rows) {   // (row >= 0: a row of tile_rows)
        vb = p.vert_offsets[row];
        ve = p.vert_offsets[row + 1];
        vb = vb < 0 ? 0 : (vb > p.n_verts ? p.n_verts : vb);
        ve = ve < vb ? vb : (ve > p.n_verts ? p.n_verts : ve);
    }
}

struct Affine { double m00, m01, m02, m10, m11, m12; };

// One wave, one polygon (k vertices from vb; mirror: a pasted polygon) at position j: resample, warp, segment2box -> boxes[j], inside[j]; returns its path bits.
Y3_DEV int polygon_row(const PolyTables& p, long long vb, int k, float wf, float hf, float lpadw, float lpadh, float c, bool mirror, const Affine& M, double Sd, int lane, long long j) {
    int flags = 0;
    bool nonzero = false, anyx = false;
    double x1 = 0, y1 = 0, x2 = 0, y2 = 0;
    bool have = false;
    if (k == 0) {
        flags |= PATH_LACKS;
    } else {
        for (int v = lane; v < k; v += 64) {
            float x, y;
            canvas_vertex(p.verts, vb + v, wf, hf, lpadw, lpadh, c, x, y, mirror);
            nonzero = nonzero || x != 0.0f || y != 0.0f;
        }
        const double step = (double)k / (double)(SAMPLES - 1);
        for (int i = lane; i < SAMPLES; i += 64) {
            const double x = i == SAMPLES - 1 ? (double)k : (double)i * step;
            int q = (int)x;
            q = q > k ? k : q;
            const int q0 = q == k ? 0 : q;   // the closing vertex
            float ax, ay;
            canvas_vertex(p.verts, vb + q0, wf, hf, lpadw, lpadh, c, ax, ay, mirror);
            double px = (double)ax, py = (double)ay;
            if (q < k && x != (double)q) {
                float bx, by;
                canvas_vertex(p.verts, vb + (q + 1 == k ? 0 : q + 1), wf, hf, lpadw, lpadh, c, bx, by, mirror);
                const double f = x - (double)q;
                px = ((double)bx - px) * f + px;
                py = ((double)by - py) * f + py;
            }
            const double X = px * M.m00 + py * M.m01 + M.m02, Y = px * M.m10 + py * M.m11 + M.m12;
            if (X >= 0.0 && Y >= 0.0 && X <= Sd && Y <= Sd) {
                x1 = !have || X < x1 ? X : x1; x2 = !have || X > x2 ? X : x2;
                y1 = !have || Y < y1 ? Y : y1; y2 = !have || Y > y2 ? Y : y2;
                have = true;
                anyx = anyx || X != 0.0;
            }
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const double ox1 = __shfl_xor(x1, d), oy1 = __shfl_xor(y1, d), ox2 = __shfl_xor(x2, d), oy2 = __shfl_xor(y2, d);
        const int oh = __shfl_xor((int)have, d);
        if (oh) {
            x1 = !have || ox1 < x1 ? ox1 : x1; x2 = !have || ox2 > x2 ? ox2 : x2;
            y1 = !have || oy1 < y1 ? oy1 : y1; y2 = !have || oy2 > y2 ? oy2 : y2;
            have = true;
        }
    }
    if (__any(nonzero)) flags |= PATH_NONZERO;
    const bool taken = __any(anyx) != 0;   // segment2box's any(x): with no kept point, or every kept X zero, the box is zeros
    if (lane == 0 && j < p.ws_rows) {
        double* o = p.boxes + j * 4;
        o[0] = taken ? x1 : 0.0; o[1] = taken ? y1 : 0.0; o[2] = taken ? x2 : 0.0; o[3] = taken ? y2 : 0.0;
        p.inside[j] = taken ? 1 : 0;
    }
    return flags;
}

// One block per (item, mosaic), one wave per label row at a time: the rows of the mosaic's tiles in tile order, at the positions j augment_targets_kernel gives them (the
// label counts of every slot before the mosaic are summed by the block).  A lane takes samples lane, lane + 64, ... of the 1000 of np.linspace(0, k, 1000) over the
// closed polygon (vertex k is vertex 0), interpolates as np.interp does in fp64 -- (b - a) (x - j) + a, a itself where x == j -- forms X = x m00 + y m01 + m02 and Y
// likewise as plain sums, keeps the points with 0 <= X, Y <= S, and the wave reduces min / max.  Vertices are read by index from the table, never staged: a polygon may
// have more vertices than samples.  Mosaics of the letterbox branch (clip == 0) hand no segments to random_perspective: their word is 0 and their rows are not touched.
// CP: the k paste positions of the mosaic follow its tile rows; an accepted one carries polygon j mirrored (fp32(2 s) - x of the clipped vertex), formed on the fly,
// and counts in the path word, which is thus formed over the segments after the paste; an unaccepted one is a dropped row (a zero box, no bit).
template <bool CP> __global__ __launch_bounds__(BT) void augment_polygons_kernel(const TargetArgs a, const PolyTables p, const PasteTables cp) {
    __shared__ long long s_sum[BT / 64];
    __shared__ int s_flag[BT / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, mslot = blockIdx.x, b = mslot >> 1, m = mslot & 1;
    const long long total = a.label_offsets[a.n_images];
    long long before = 0;
    for (int s = tid; s < mslot * 4; s += BT) {
        long long beg, end;
        tile_rows(a, total, s, beg, end);
        before += end - beg;
    }
    if constexpr (CP) {
        for (int s = tid; s < mslot; s += BT) {
            int kb, kk;
            paste_range(cp, s, kb, kk);
            before += kk;
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) before += __shfl_xor(before, d);
    if (lane == 0) s_sum[wave] = before;
    __syncthreads();
    long long base = 0;
#pragma unroll
    for (int w = 0; w < BT / 64; ++w) base += s_sum[w];
    base = base > 0x3fffffff ? 0x3fffffff : base;   // (the saturating prefix of augment_targets_kernel)
    const y3_augment_item* it = a.items + b;
    const y3_augment_mosaic* mo = &it->mosaics[m];
    if (m >= clampi(it->nmos, 0, 2) || !mo->clip) {
        if (tid == 0) p.paths[mslot] = 0;
        return;
    }
    const int ntiles = clampi(mo->ntiles, 0, 4);
    const float c = (float)mo->canvas;
    const double Sd = (double)a.W;   // (square only: H == W)
    const Affine M = {mo->m[0], mo->m[1], mo->m[2], mo->m[3], mo->m[4], mo->m[5]};
    int flags = 0;
    for (int t = 0; t < ntiles; ++t) {
        long long beg, end;
        tile_rows(a, total, mslot * 4 + t, beg, end);
        if (end > beg) {
            const y3_augment_tile tl = mo->tiles[t];
            const y3_dataset_image im = a.images[tl.img];   // (tile_rows found the image inside the table)
            const float wf = (float)im.w, hf = (float)im.h;
            for (long long r = wave; r < end - beg; r += BT / 64) {
                long long vb, ve;
                row_vertices(p, beg + r, vb, ve);
                flags |= polygon_row(p, vb, (int)(ve - vb), wf, hf, tl.lpadw, tl.lpadh, c, false, M, Sd, lane, base + r);   // n_verts < 2^31
            }
        }
        base += end - beg;
    }
    if constexpr (CP) {
        int kb, kk;
        paste_range(cp, mslot, kb, kk);
        for (int e = wave; e < kk; e += BT / 64) {
            const int* si = cp.sel_i + (long long)(kb + e) * 4;
            const int t = si[3];
            long long beg = 0, end = 0, vb = 0, ve = 0;
            if (si[0] && t >= 0 && t < ntiles) tile_rows(a, total, mslot * 4 + t, beg, end);
            if (si[2] >= beg && si[2] < end) row_vertices(p, si[2], vb, ve);
            if (ve > vb) {
                const y3_augment_tile tl = mo->tiles[t];
                const y3_dataset_image im = a.images[tl.img];
                flags |= polygon_row(p, vb, (int)(ve - vb), (float)im.w, (float)im.h, tl.lpadw, tl.lpadh, c, true, M, Sd, lane, base + e);
            } else if (lane == 0 && base + e < p.ws_rows) {
                double* o = p.boxes + (base + e) * 4;
                o[0] = o[1] = o[2] = o[3] = 0.0;
                p.inside[base + e] = 0;
            }
        }
    }
    if (lane == 0) s_flag[wave] = flags;
    __syncthreads();
    if (tid == 0) {
        int f = 0;
#pragma unroll
        for (int w = 0; w < BT / 64; ++w) f |= s_flag[w];
        p.paths[mslot] = f;
    }
}

// ONE block per batch.  The prefix of the label counts of the batch's tiles (item, mosaic, tile: the reference's order) lives in LDS; the block walks the rows 256 at
// a time: a lane transforms one label and decides whether box_candidates keeps it, a ballot and the waves' counts give every survivor its place behind the
// survivors before it, and the per-item counts become the bs + 1 offsets.  Survivors past n_rows are dropped (and not counted).
// POLY: a row of a mosaic whose word is PATH_NONZERO takes the box augment_polygons_kernel left at its position (no further clip) and area_thr 0.01; every other row,
// and every row of the plain form, runs the four-corner arithmetic.
// CP (with POLY): the k paste positions of a mosaic are counted with the rows of its fourth tile and follow them; an accepted one is the appended label row of
// sel_f, every other a dropped row.
template <bool POLY, bool CP> __global__ __launch_bounds__(BT) void augment_targets_kernel(const TargetArgs a, const PolyTables p, const PasteTables cp) {
    __shared__ int s_pref[MAX_BS * SLOTS + 1];
    __shared__ int s_cnt[MAX_BS];
    __shared__ int s_wave[BT / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nslots = a.count * SLOTS;
    const long long total = a.label_offsets[a.n_images];
    for (int s = tid; s < nslots; s += BT) {
        long long beg, end;
        tile_rows(a, total, s, beg, end);
        int extra = 0;
        if constexpr (CP) {
            int kb;
            if ((s & 3) == 3) paste_range(cp, s >> 2, kb, extra);
        }
        s_pref[s + 1] = (int)(end - beg) + extra;
    }
    for (int b = tid; b < a.count; b += BT) s_cnt[b] = 0;
    __syncthreads();
    if (tid == 0) {
        int run = 0;
        s_pref[0] = 0;
        for (int s = 0; s < nslots; ++s) {
            const int n = s_pref[s + 1];
            run = run > 0x3fffffff - n ? 0x3fffffff : run + n;
            s_pref[s + 1] = run;
        }
    }
    __syncthreads();
    const int have = s_pref[nslots];
    const float Wf = (float)a.W, Hf = (float)a.H;
    const double Wd = (double)a.W, Hd = (double)a.H;
    long long running = 0;
    for (int base = 0; base < have; base += BT) {
        const int j = base + tid;
        bool keep = false;
        int b = 0;
        float cls = 0.0f, ox = 0.0f, oy = 0.0f, ow = 0.0f, oh = 0.0f;
        if (j < have) {
            int lo = 0, hi = nslots - 1;   // the last slot with s_pref[slot] <= j
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if (s_pref[mid] <= j) lo = mid;
                else hi = mid - 1;
            }
            long long beg, end;
            tile_rows(a, total, lo, beg, end);
            const long long row = beg + (j - s_pref[lo]);
            bool have_row = false;
            float x1 = 0.0f, y1 = 0.0f, x2 = 0.0f, y2 = 0.0f;
            const y3_augment_item* it = a.items + (lo >> 3);
            const y3_augment_mosaic* mo = &it->mosaics[(lo >> 2) & 1];
            if (row < end) {
                const y3_augment_tile tl = mo->tiles[lo & 3];
                const y3_dataset_image im = a.images[tl.img];
                const float* l = a.labels + row * 5;
                cls = l[0];
                canvas_box(mo, tl, im, l, x1, y1, x2, y2);
                have_row = true;
            } else if constexpr (CP) {
                int kb, kk;
                paste_range(cp, lo >> 2, kb, kk);
                const long long e = row - end;
                if (e < kk && cp.sel_i[(kb + e) * 4]) {
                    const float* f = cp.sel_f + (kb + e) * 5;
                    cls = f[0]; x1 = f[1]; y1 = f[2]; x2 = f[3]; y2 = f[4];
                    have_row = true;
                }
            }
            if (have_row) {
                b = lo >> 3;
                // the four corners through M in fp64, each coordinate a plain left-to-right sum of three terms
                const double m00 = mo->m[0], m01 = mo->m[1], m02 = mo->m[2], m10 = mo->m[3], m11 = mo->m[4], m12 = mo->m[5];
                const double px[4] = {(double)x1, (double)x2, (double)x1, (double)x2}, py[4] = {(double)y1, (double)y2, (double)y2, (double)y1};
                double nx1 = 0, ny1 = 0, nx2 = 0, ny2 = 0;
                bool poly = false;
                if constexpr (POLY) poly = p.paths[(lo >> 2)] == PATH_NONZERO;   // (lo >> 2 is item * 2 + mosaic)
                if (poly) {   // segment2box of the warped polygon (all zeros without a point inside: the row fails w2 > 2)
                    if (j < p.ws_rows && p.inside[j]) {
                        const double* q = p.boxes + (long long)j * 4;
                        nx1 = q[0]; ny1 = q[1]; nx2 = q[2]; ny2 = q[3];
                    }
                } else {
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const double X = px[q] * m00 + py[q] * m01 + m02, Y = px[q] * m10 + py[q] * m11 + m12;
                        nx1 = q == 0 || X < nx1 ? X : nx1; nx2 = q == 0 || X > nx2 ? X : nx2;
                        ny1 = q == 0 || Y < ny1 ? Y : ny1; ny2 = q == 0 || Y > ny2 ? Y : ny2;
                    }
                    nx1 = nx1 < 0.0 ? 0.0 : nx1; nx1 = nx1 > Wd ? Wd : nx1;
                    nx2 = nx2 < 0.0 ? 0.0 : nx2; nx2 = nx2 > Wd ? Wd : nx2;
                    ny1 = ny1 < 0.0 ? 0.0 : ny1; ny1 = ny1 > Hd ? Hd : ny1;
                    ny2 = ny2 < 0.0 ? 0.0 : ny2; ny2 = ny2 > Hd ? Hd : ny2;
                }
                // box_candidates(box1 = targets * s (fp32), box2 = new (fp64), wh_thr 2, ar_thr 100, area_thr 0.1 (0.01 on the polygon path), eps 1e-16)
                const float sc = (float)mo->scale;
                const float w1 = x2 * sc - x1 * sc, h1 = y2 * sc - y1 * sc;
                const double w2 = nx2 - nx1, h2 = ny2 - ny1, eps = 1e-16;
                const double r1 = w2 / (h2 + eps), r2 = h2 / (w2 + eps), ar = r1 > r2 ? r1 : r2;
                const float den = w1 * h1 + (float)eps;
                keep = w2 > 2.0 && h2 > 2.0 && w2 * h2 / (double)den > (poly ? 0.01 : 0.1) && ar < 100.0;
                // the survivor as fp32, xyxy2xywhn(clip=True, eps=1e-3), the flips
                float fx1 = (float)nx1, fy1 = (float)ny1, fx2 = (float)nx2, fy2 = (float)ny2;
                fx1 = fx1 < 0.0f ? 0.0f : fx1; fx1 = fx1 > a.clip_w ? a.clip_w : fx1;
                fx2 = fx2 < 0.0f ? 0.0f : fx2; fx2 = fx2 > a.clip_w ? a.clip_w : fx2;
                fy1 = fy1 < 0.0f ? 0.0f : fy1; fy1 = fy1 > a.clip_h ? a.clip_h : fy1;
                fy2 = fy2 < 0.0f ? 0.0f : fy2; fy2 = fy2 > a.clip_h ? a.clip_h : fy2;
                ox = ((fx1 + fx2) / 2.0f) / Wf;
                oy = ((fy1 + fy2) / 2.0f) / Hf;
                ow = (fx2 - fx1) / Wf;
                oh = (fy2 - fy1) / Hf;
                if (it->flipud) oy = 1.0f - oy;
                if (it->fliplr) ox = 1.0f - ox;
            }
        }
        const unsigned long long vote = __ballot(keep);
        if (lane == 0) s_wave[wave] = __popcll(vote);
        __syncthreads();
        int before = __popcll(vote & ((1ull << lane) - 1ull)), all = 0;
#pragma unroll
        for (int w = 0; w < BT / 64; ++w) {
            before += w < wave ? s_wave[w] : 0;
            all += s_wave[w];
        }
        const long long pos = running + before;
        if (keep && pos < a.n_rows) {
            float* o = a.out + pos * 6;
            o[0] = (float)b; o[1] = cls; o[2] = ox; o[3] = oy; o[4] = ow; o[5] = oh;
            atomicAdd(&s_cnt[b], 1);
        }
        running += all;
        __syncthreads();
    }
    if (tid == 0) {
        long long run = 0;
        a.out_offsets[0] = 0;
        for (int b = 0; b < a.count; ++b) {
            run += s_cnt[b];
            a.out_offsets[b + 1] = run;
        }
    }
}

// bbox_ioa of one box against one label row, fp32: the intersection, clip(0) per axis, over area(row) + 1e-7
Y3_DEV float box_ioa(float bx1, float by1, float bx2, float by2, float lx1, float ly1, float lx2, float ly2) {
    float iw = fminf(bx2, lx2) - fmaxf(bx1, lx1), ih = fminf(by2, ly2) - fmaxf(by1, ly1);
    iw = iw < 0.0f ? 0.0f : iw;
    ih = ih < 0.0f ? 0.0f : ih;
    return iw * ih / ((lx2 - lx1) * (ly2 - ly1) + 1e-7f);
}

// Copy-paste's selection: one block per (item, mosaic) with k > 0.  The block walks js serially; for candidate j, label row j of labels4 (the rows of the four tiles
// in tile order, canvas_box) gives box = (w - x2, y1, w - x1, y2), the lanes stride over all current rows -- the tile rows and the rows appended by earlier
// candidates, read back from sel_f -- and the block ORs "some ioa is not < 0.30".  Polygon j is polygon j of segments4: the rows of the tiles whose image has polygons
// (an image has one per row or none: pack_polygons), so in a mosaic that mixes polygon and box-only images it is not the polygon of label row j.
__global__ __launch_bounds__(BT) void copy_paste_select_kernel(const TargetArgs a, const PolyTables p, const PasteTables cp) {
    __shared__ long long s_beg[4];
    __shared__ int s_rows[4], s_poly[4];
    const int tid = threadIdx.x, mslot = blockIdx.x, b = mslot >> 1, m = mslot & 1;
    int kb, kk;
    paste_range(cp, mslot, kb, kk);
    if (kk == 0) return;
    const y3_augment_item* it = a.items + b;
    const y3_augment_mosaic* mo = &it->mosaics[m];
    if (m >= clampi(it->nmos, 0, 2) || !mo->clip || mo->ntiles != 4) {   // (the host gives such a mosaic no candidates)
        for (int e = tid; e < kk; e += BT) cp.sel_i[(long long)(kb + e) * 4] = 0;
        return;
    }
    const long long total = a.label_offsets[a.n_images];
    if (tid < 4) {
        long long beg, end, vb = 0, ve = 0;
        tile_rows(a, total, mslot * 4 + tid, beg, end);
        if (end > beg) row_vertices(p, beg, vb, ve);
        s_beg[tid] = beg;
        s_rows[tid] = (int)(end - beg);
        s_poly[tid] = ve > vb ? (int)(end - beg) : 0;
    }
    __syncthreads();
    const int nrows = s_rows[0] + s_rows[1] + s_rows[2] + s_rows[3], npoly = s_poly[0] + s_poly[1] + s_poly[2] + s_poly[3];
    const int* js = cp.table + 4 * a.count + 1;
    const float w = (float)mo->canvas;
    // row r of labels4 -> (cls, x1, y1, x2, y2)
    auto row_box = [&](int r, float& cls, float& x1, float& y1, float& x2, float& y2) {
        int t = 0;
        while (t < 3 && r >= s_rows[t]) r -= s_rows[t++];
        const y3_augment_tile tl = mo->tiles[t];
        const float* l = a.labels + (s_beg[t] + r) * 5;
        cls = l[0];
        canvas_box(mo, tl, a.images[tl.img], l, x1, y1, x2, y2);
    };
    for (int e = 0; e < kk; ++e) {
        const int j = js[kb + e];
        const bool ok = j >= 0 && j < npoly && j < nrows;   // (uniform over the block)
        float cls = 0.0f, bx1 = 0.0f, by1 = 0.0f, bx2 = 0.0f, by2 = 0.0f;
        int prow = 0, ptile = 0, bad = 1;
        if (ok) {
            float x1, y1, x2, y2;
            row_box(j, cls, x1, y1, x2, y2);
            bx1 = w - x2; by1 = y1; bx2 = w - x1; by2 = y2;
            int q = j;
            while (ptile < 3 && q >= s_poly[ptile]) q -= s_poly[ptile++];
            prow = (int)(s_beg[ptile] + q);
            bad = 0;
            for (int r = tid; r < nrows; r += BT) {
                float c2, lx1, ly1, lx2, ly2;
                row_box(r, c2, lx1, ly1, lx2, ly2);
                bad |= !(box_ioa(bx1, by1, bx2, by2, lx1, ly1, lx2, ly2) < 0.30f);
            }
            for (int r = tid; r < e; r += BT) {
                if (cp.sel_i[(long long)(kb + r) * 4]) {
                    const float* f = cp.sel_f + (long long)(kb + r) * 5;
                    bad |= !(box_ioa(bx1, by1, bx2, by2, f[1], f[2], f[3], f[4]) < 0.30f);
                }
            }
        }
        const int refused = __syncthreads_or(bad);
        if (tid == 0) {
            int* si = cp.sel_i + (long long)(kb + e) * 4;
            float* sf = cp.sel_f + (long long)(kb + e) * 5;
            si[0] = refused ? 0 : 1; si[1] = j; si[2] = prow; si[3] = ptile;
            sf[0] = cls; sf[1] = bx1; sf[2] = by1; sf[3] = bx2; sf[4] = by2;
        }
        __threadfence_block();
        __syncthreads();   // the next candidate reads this one's row
    }
}

constexpr int EDGE_CAP = 1024;   // the edges of a polygon kept in LDS (24 KB); a longer polygon forms the rest from its vertices at every use

struct Edge { long long x, dx; int y0, y1; };   // y0 <= y < y1, x at y0 in 16.16, dx per line; a horizontal edge has y0 == y1 and is never active

Y3_DEV Edge make_edge(int xa, int ya, int xb, int yb) {
    Edge e;
    if (ya > yb) { const int tx = xa, ty = ya; xa = xb; ya = yb; xb = tx; yb = ty; }
    e.y0 = ya; e.y1 = yb; e.x = (long long)xa * 65536; e.dx = 0;
    if (yb > ya) e.dx = ((long long)(xb - xa) * 65536) / (long long)(yb - ya);   // truncates towards zero
    return e;
}

Y3_DEV void set_bit(unsigned* mask, int words, int x, int y) { atomicOr(mask + (long long)y * words + (x >> 5), 1u << (x & 31)); }

// the 8-connected line of drawContours' boundary on a w x w image: cv::clipLine, then LineIterator's stepping from the end with the smaller x
Y3_DEV void draw_line(unsigned* mask, int w, int words, long long x1, long long y1, long long x2, long long y2) {
    const long long right = w - 1, bottom = w - 1;
    int c1 = (x1 < 0) + (x1 > right) * 2 + (y1 < 0) * 4 + (y1 > bottom) * 8, c2 = (x2 < 0) + (x2 > right) * 2 + (y2 < 0) * 4 + (y2 > bottom) * 8;
    if ((c1 & c2) == 0 && (c1 | c2) != 0) {
        long long q;
        if (c1 & 12) {
            q = c1 < 8 ? 0 : bottom;
            x1 += (long long)((double)(q - y1) * (double)(x2 - x1) / (double)(y2 - y1));
            y1 = q;
            c1 = (x1 < 0) + (x1 > right) * 2;
        }
        if (c2 & 12) {
            q = c2 < 8 ? 0 : bottom;
            x2 += (long long)((double)(q - y2) * (double)(x2 - x1) / (double)(y2 - y1));
            y2 = q;
            c2 = (x2 < 0) + (x2 > right) * 2;
        }
        if ((c1 & c2) == 0 && (c1 | c2) != 0) {
            if (c1) {
                q = c1 == 1 ? 0 : right;
                y1 += (long long)((double)(q - x1) * (double)(y2 - y1) / (double)(x2 - x1));
                x1 = q;
                c1 = 0;
            }
            if (c2) {
                q = c2 == 1 ? 0 : right;
                y2 += (long long)((double)(q - x2) * (double)(y2 - y1) / (double)(x2 - x1));
                x2 = q;
                c2 = 0;
            }
        }
    }
    if ((c1 | c2) != 0 || x1 < 0 || x1 > right || x2 < 0 || x2 > right || y1 < 0 || y1 > bottom || y2 < 0 || y2 > bottom) return;   // (nothing is set outside the mask)
    if (x2 < x1) { long long t = x1; x1 = x2; x2 = t; t = y1; y1 = y2; y2 = t; }
    const int dx = (int)(x2 - x1), dy = (int)(y2 > y1 ? y2 - y1 : y1 - y2), sy = y2 < y1 ? -1 : 1;
    const bool steep = dy > dx;
    const int major = steep ? dy : dx, minor = steep ? dx : dy;
    int err = major - 2 * minor, x = (int)x1, y = (int)y1;
    for (int i = 0; i <= major; ++i) {
        set_bit(mask, words, x, y);
        const bool neg = err < 0;
        err += -2 * minor + (neg ? 2 * major : 0);
        if (steep) { y += sy; x += neg ? 1 : 0; }
        else { x += 1; y += neg ? sy : 0; }
    }
}

// Copy-paste's raster: one block per accepted slot fills polygon j -- its vertices by index through xyn2xy, the clip and the truncation of astype(int32) -- into the
// 1-bit mask of its mosaic as tests/augment_copy_paste_cases.py::fill_mask states drawContours(FILLED).  A lane draws the boundary lines of vertices lane, lane + 256,
// ...; then an (y, word) pair of the polygon's bounding box per lane at a time: over the edges active at y the pixels right of an odd number of crossings, that is
// with P = px << 16 the parity of the crossings x < P -- the spans (x_left + 65535) >> 16 .. x_right >> 16 of the sorted pairs without the sort -- and the pixels
// with a crossing at P itself.  Everything goes in with atomicOr: slots of one mosaic share its mask.
__global__ __launch_bounds__(BT) void copy_paste_raster_kernel(const TargetArgs a, const PolyTables p, const PasteTables cp) {
    __shared__ Edge s_edge[EDGE_CAP];
    __shared__ int s_box[4];   // min x, min y, max x, max y
    const int tid = threadIdx.x, g = blockIdx.x;
    const int* si = cp.sel_i + (long long)g * 4;
    if (!si[0]) return;
    int lo = 0, hi = 2 * a.count - 1;   // the last mosaic whose slots begin at or before g
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (cp.table[mid] <= g) lo = mid;
        else hi = mid - 1;
    }
    const int mslot = lo, t = si[3], mi = cp.table[2 * a.count + 1 + mslot];
    int kb, kk;
    paste_range(cp, mslot, kb, kk);
    const y3_augment_item* it = a.items + (mslot >> 1);
    const y3_augment_mosaic* mo = &it->mosaics[mslot & 1];
    const int w = 2 * a.W, words = w >> 5;
    if (g < kb || g >= kb + kk || mi < 0 || mi >= cp.n_masks || t < 0 || t > 3 || (mslot & 1) >= clampi(it->nmos, 0, 2) || !mo->clip || mo->ntiles != 4 || mo->canvas != w) return;
    const long long total = a.label_offsets[a.n_images];
    long long beg, end, vb = 0, ve = 0;
    tile_rows(a, total, mslot * 4 + t, beg, end);
    if (si[2] >= beg && si[2] < end) row_vertices(p, si[2], vb, ve);
    const int nv = (int)(ve - vb);
    if (nv < 1) return;
    const y3_augment_tile tl = mo->tiles[t];
    const y3_dataset_image im = a.images[tl.img];
    const float wf = (float)im.w, hf = (float)im.h, c = (float)w;
    unsigned* mask = cp.masks + (long long)mi * w * words;
    auto vertex = [&](int i, int& x, int& y) {
        float fx, fy;
        canvas_vertex(p.verts, vb + i, wf, hf, tl.lpadw, tl.lpadh, c, fx, fy);
        x = (int)fx; y = (int)fy;
    };
    if (tid == 0) { s_box[0] = s_box[1] = 0x7fffffff; s_box[2] = s_box[3] = -1; }
    __syncthreads();
    for (int i = tid; i < nv; i += BT) {
        int x0, y0, x1, y1;
        vertex(i == 0 ? nv - 1 : i - 1, x0, y0);
        vertex(i, x1, y1);
        draw_line(mask, w, words, x0, y0, x1, y1);
        if (i < EDGE_CAP) s_edge[i] = make_edge(x0, y0, x1, y1);
        atomicMin(&s_box[0], x1); atomicMin(&s_box[1], y1); atomicMax(&s_box[2], x1); atomicMax(&s_box[3], y1);
    }
    __syncthreads();
    const int ymin = s_box[1], ymax = s_box[3] < w ? s_box[3] : w, w0 = s_box[0] >> 5, w1 = (s_box[2] < w ? s_box[2] : w - 1) >> 5;   // rows ymin <= y < ymax
    const int nw = w1 - w0 + 1, n = (ymax - ymin) * nw;
    for (int i = tid; i < n; i += BT) {
        const int y = ymin + i / nw, wd = w0 + i % nw;
        const long long first = (long long)wd * 32;
        unsigned odd = 0u, at = 0u;
        for (int e = 0; e < nv; ++e) {
            Edge ed;
            if (e < EDGE_CAP) ed = s_edge[e];
            else {
                int x0, y0, x1, y1;
                vertex(e - 1, x0, y0);
                vertex(e, x1, y1);
                ed = make_edge(x0, y0, x1, y1);
            }
            if (ed.y0 <= y && y < ed.y1) {
                const long long x = ed.x + (long long)(y - ed.y0) * ed.dx;
                const long long rel = (x >> 16) + 1 - first;   // the first pixel of this word right of the crossing
                if (rel <= 0) odd = ~odd;
                else if (rel < 32) odd ^= 0xffffffffu << rel;
                const long long q = (x >> 16) - first;
                if ((x & 0xffff) == 0 && q >= 0 && q < 32) at |= 1u << q;
            }
        }
        const unsigned bits = odd | at;
        if (bits) atomicOr(mask + (long long)y * words + wd, bits);
    }
}

// ---- the host side.  An export copies its arguments into the structs its kernel takes (nothing is tested on the way) and hands them to the launcher of its kernel
// family, which refuses in the order every export has kept -- a null pointer, the set and the paste table (check_set), a count, an alignment -- with the family's texts
// under the export's own name, and launches.
bool aligned(const void* p, uintptr_t n) { return ((uintptr_t)p & (n - 1)) == 0; }

TargetArgs target_args(const float* labels, const int64_t* label_offsets, const y3_dataset_image* images, int64_t n_images, const y3_augment_item* items, int32_t count,
                       int32_t H, int32_t W, float* targets = nullptr, int64_t n_rows = 0, int64_t* offsets = nullptr) {
    TargetArgs a = {};
    a.labels = labels; a.label_offsets = (const long long*)label_offsets; a.images = images; a.n_images = n_images; a.items = items;
    a.out = targets; a.n_rows = n_rows; a.out_offsets = (long long*)offsets; a.count = count; a.H = H; a.W = W;
    a.clip_w = (float)((double)W - 1e-3);
    a.clip_h = (float)((double)H - 1e-3);
    return a;
}

// PolyTables and PasteTables are filled in place, in the order of their fields (a form leaves out the tail it does not read).  What more than one family tests:
// the extents of the vertex table (at least `least` vertices), a row count, the fp64 / int32 workspace of the polygon kernel
bool bad_vertex_table(const PolyTables& p, long long least = 0) { return p.n_verts < least || p.n_verts > 0x7fffffffLL / 2 || p.n_vert_rows < 0 || p.n_vert_rows > 0x7fffffffLL; }
bool bad_rows(long long n) { return n < 0 || n > 0x7fffffffLL / 6; }
bool null_workspace(const PolyTables& p, int count) { return (count > 0 && !p.paths) || (p.ws_rows > 0 && (!p.boxes || !p.inside)); }
bool misaligned_workspace(const PolyTables& p) { return !aligned(p.boxes, 8) || !aligned(p.inside, 4) || !aligned(p.paths, 4); }

enum SelReads { SEL_I_AND_F, SEL_I_ONLY };   // what a copy-paste form reads of the selection: the raster reads sel_i alone

// the set every export takes (images, items, count, H, W of `a`) and, for a copy-paste form, the table of the batch `c` and what the selection leaves
int check_set(const char* fn, const TargetArgs& a, const PasteTables* c = nullptr, SelReads reads = SEL_I_AND_F) {
    if (!a.images || !a.items) Y3_FAIL("%s: null argument", fn);
    if (a.n_images < 1 || a.n_images > 0x7fffffffLL || a.count < 0 || a.count > MAX_BS || a.H < 16 || a.H > MAX_S || a.W < 16 || a.W > MAX_S)
        Y3_FAIL("%s: bad geometry (%lld images in 1 .. 2^31 - 1, a batch of %d in 0 .. %d items of %d x %d in 16 .. %d)", fn, a.n_images, a.count, MAX_BS, a.H, a.W, MAX_S);
    if (a.H % 16) Y3_FAIL("%s: the image size %d is not a multiple of 16", fn, a.H);
    if (a.W % 16) Y3_FAIL("%s: the image size %d is not a multiple of 16", fn, a.W);
    if (!aligned(a.images, 8) || !aligned(a.items, 8)) Y3_FAIL("%s: the record table and the items must be 8-byte aligned", fn);
    if (!c) return 0;
    if (!c->table || !c->sel_i || (reads == SEL_I_AND_F && !c->sel_f)) Y3_FAIL("%s: null argument", fn);
    if (c->nk < 1 || c->nk > 0x3fffffff / 6) Y3_FAIL("%s: bad geometry (%d candidates)", fn, c->nk);
    if (a.W % 16 || 2 * a.W % 32) Y3_FAIL("%s: the canvas 2 x %d is not a multiple of 32", fn, a.W);
    if (!aligned(c->table, 4) || !aligned(c->sel_i, 4) || !aligned(c->sel_f, 4)) Y3_FAIL("%s: the int32 and fp32 tables must be 4-byte aligned", fn);
    return 0;
}

template <typename A> void launch_sampler(int32_t dst_dtype, dim3 grid, hipStream_t st, const A& a) {
    switch (dst_dtype) {
        case Y3_U8: hipLaunchKernelGGL((augment_batch_kernel<unsigned char, A>), grid, dim3(BT), 0, st, a); break;
        case Y3_F16: hipLaunchKernelGGL((augment_batch_kernel<f16_t, A>), grid, dim3(BT), 0, st, a); break;
        case Y3_BF16: hipLaunchKernelGGL((augment_batch_kernel<bf16_t, A>), grid, dim3(BT), 0, st, a); break;
        default: hipLaunchKernelGGL((augment_batch_kernel<float, A>), grid, dim3(BT), 0, st, a); break;
    }
}

int launch_batch(const char* fn, const uint8_t* arena, int64_t arena_bytes, const y3_dataset_image* images, int64_t n_images, const y3_augment_item* items, int32_t count,
                 void* dst, int32_t dst_dtype, int32_t H, int32_t W, void* stream, const int32_t* paste = nullptr, const int32_t* masks = nullptr, int32_t n_masks = 0) {
    if (!arena || !dst) Y3_FAIL("%s: null argument", fn);
    if (check_set(fn, target_args(nullptr, nullptr, images, n_images, items, count, H, W))) return -1;
    if (arena_bytes < 4 || (arena_bytes & 3)) Y3_FAIL("%s: the arena's %lld bytes are not a positive multiple of 4", fn, (long long)arena_bytes);
    if (!aligned(arena, 16) || !aligned(dst, 16)) Y3_FAIL("%s: the arena and the output must be 16-byte aligned", fn);
    if (dst_dtype != Y3_U8 && dst_dtype != Y3_F16 && dst_dtype != Y3_BF16 && dst_dtype != Y3_F32) Y3_FAIL("%s: unsupported output dtype %d (uint8 / float16 / bfloat16 / float32)", fn, dst_dtype);
    if (count == 0) return 0;
    BatchPasteArgs a;
    a.arena = arena; a.arena_bytes = arena_bytes; a.images = images; a.n_images = n_images; a.items = items; a.dst = dst;
    a.count = count; a.H = H; a.W = W; a.pixels = H * W;   // <= 2^24, a multiple of 256
    a.w_div = y3_make_divisor(W);
    a.paste = paste; a.masks = (const unsigned*)masks; a.n_masks = n_masks;
    const dim3 grid((unsigned)((a.pixels + CHUNK - 1) / CHUNK), (unsigned)count);
    if (paste) launch_sampler<BatchPasteArgs>(dst_dtype, grid, (hipStream_t)stream, a);
    else launch_sampler<BatchArgs>(dst_dtype, grid, (hipStream_t)stream, a);
    Y3_CHECK_LAUNCH();
    return 0;
}

// y3_augment_polygons and, with the paste table `c`, y3_augment_polygons_paste
int launch_polygons(const char* fn, const TargetArgs& a, const PolyTables& p, const PasteTables* c, void* stream) {
    if (!p.vert_offsets || !a.label_offsets || null_workspace(p, a.count) || (p.n_verts > 0 && !p.verts)) Y3_FAIL("%s: null argument", fn);
    if (check_set(fn, a, c)) return -1;
    if (bad_vertex_table(p) || bad_rows(p.ws_rows)) Y3_FAIL("%s: bad geometry (%lld vertices, %lld label rows, a workspace of %lld rows)", fn, p.n_verts, p.n_vert_rows, p.ws_rows);
    if (!aligned(p.vert_offsets, 8) || !aligned(a.label_offsets, 8) || !aligned(p.verts, 4) || misaligned_workspace(p))
        Y3_FAIL("%s: the offsets and the boxes must be 8-byte, the vertices and the int32 words 4-byte aligned", fn);
    if (a.count == 0) return 0;
    const dim3 grid((unsigned)a.count * 2);
    if (c) hipLaunchKernelGGL(augment_polygons_kernel<true>, grid, dim3(BT), 0, (hipStream_t)stream, a, p, *c);
    else hipLaunchKernelGGL(augment_polygons_kernel<false>, grid, dim3(BT), 0, (hipStream_t)stream, a, p, PasteTables{});
    Y3_CHECK_LAUNCH();
    return 0;
}

// the four targets exports: the box form; with the workspace `p` the polygon form; with the paste table `c` besides (never without `p`), the copy-paste form.  One
// block, for an empty batch too: it writes offsets[0].
int launch_targets(const char* fn, const TargetArgs& a, const PolyTables* p, const PasteTables* c, void* stream) {
    if (!a.label_offsets || !a.out_offsets || (a.n_rows > 0 && (!a.labels || !a.out)) || (p && null_workspace(*p, a.count))) Y3_FAIL("%s: null argument", fn);
    if (check_set(fn, a, c)) return -1;
    if (bad_rows(a.n_rows)) Y3_FAIL("%s: bad geometry (%lld rows)", fn, a.n_rows);
    if (!aligned(a.label_offsets, 8) || !aligned(a.out_offsets, 8) || !aligned(a.labels, 4) || !aligned(a.out, 4) || (p && misaligned_workspace(*p)))
        Y3_FAIL(p ? "%s: the offsets and the boxes must be 8-byte, the fp32 tables and the int32 words 4-byte aligned" : "%s: the offsets must be 8-byte, the fp32 tables 4-byte aligned", fn);
    hipStream_t st = (hipStream_t)stream;
    if (c) hipLaunchKernelGGL((augment_targets_kernel<true, true>), dim3(1), dim3(BT), 0, st, a, *p, *c);
    else if (p) hipLaunchKernelGGL((augment_targets_kernel<true, false>), dim3(1), dim3(BT), 0, st, a, *p, PasteTables{});
    else hipLaunchKernelGGL((augment_targets_kernel<false, false>), dim3(1), dim3(BT), 0, st, a, PolyTables{}, PasteTables{});
    Y3_CHECK_LAUNCH();
    return 0;
}

}  // namespace

static_assert(sizeof(y3_augment_tile) == 40 && sizeof(y3_augment_mosaic) == 280 && sizeof(y3_augment_item) == 1360, "the records yolov3_amd/augment.py packs");

extern "C" int y3_augment_batch(const uint8_t* arena, int64_t arena_bytes, const y3_dataset_image* images, int64_t n_images, const y3_augment_item* items, int32_t count,
                                void* dst, int32_t dst_dtype, int32_t S, void* stream) {
    return launch_batch("y3_augment_batch", arena, arena_bytes, images, n_images, items, count, dst, dst_dtype, S, S, stream);
}

extern "C" int y3_augment_batch_hw(const uint8_t* arena, int64_t arena_bytes, const y3_dataset_image* images, int64_t n_images, const y3_augment_item* items, int32_t count,
                                   void* dst, int32_t dst_dtype, int32_t H, int32_t W, void* stream) {
    return launch_batch("y3_augment_batch_hw", arena, arena_bytes, images, n_images, items, count, dst, dst_dtype, H, W, stream);
}

extern "C" int y3_augment_batch_paste(const uint8_t* arena, int64_t arena_bytes, const y3_dataset_image* images, int64_t n_images, const y3_augment_item* items, int32_t count,
                                      void* dst, int32_t dst_dtype, int32_t S, const int32_t* paste, const int32_t* masks, int32_t n_masks, void* stream) {
    if (!paste || !masks) Y3_FAIL("y3_augment_batch_paste: null argument");
    if (n_masks < 1 || n_masks > 2 * count || 2 * S % 32 || !aligned(paste, 4) || !aligned(masks, 4)) Y3_FAIL("y3_augment_batch_paste: bad geometry (%d masks for %d items of %d) or alignment", n_masks, count, S);
    return launch_batch("y3_augment_batch_paste", arena, arena_bytes, images, n_images, items, count, dst, dst_dtype, S, S, stream, paste, masks, n_masks);
}

extern "C" int y3_augment_targets(const float* labels, const int64_t* label_offsets, const y3_dataset_image* images, int64_t n_images, const y3_augment_item* items,
                                  int32_t count, int32_t S, float* targets, int64_t n_rows, int64_t* offsets, void* stream) {
    return launch_targets("y3_augment_targets", target_args(labels, label_offsets, images, n_images, items, count, S, S, targets, n_rows, offsets), nullptr, nullptr, stream);
}

extern "C" int y3_augment_targets_hw(const float* labels, const int64_t* label_offsets, const y3_dataset_image* images, int64_t n_images, const y3_augment_item* items,
                                     int32_t count, int32_t H, int32_t W, float* targets, int64_t n_rows, int64_t* offsets, void* stream) {
    return launch_targets("y3_augment_targets_hw", target_args(labels, label_offsets, images, n_images, items, count, H, W, targets, n_rows, offsets), nullptr, nullptr, stream);
}

extern "C" int y3_augment_targets_polygons(const float* labels, const int64_t* label_offsets, const y3_dataset_image* images, int64_t n_images, const y3_augment_item* items,
                                           int32_t count, int32_t S, const double* boxes, const int32_t* inside, const int32_t* paths, float* targets, int64_t n_rows,
                                           int64_t* offsets, void* stream) {
    const PolyTables p = {nullptr, nullptr, 0, 0, const_cast<double*>(boxes), const_cast<int*>(inside), const_cast<int*>(paths), n_rows};
    return launch_targets("y3_augment_targets_polygons", target_args(labels, label_offsets, images, n_images, items, count, S, S, targets, n_rows, offsets), &p, nullptr, stream);
}

extern "C" int y3_augment_targets_paste(const float* labels, const int64_t* label_offsets, const y3_dataset_image* images, int64_t n_images, const y3_augment_item* items,
                                        int32_t count, int32_t S, const int32_t* paste, int32_t n_paste, const int32_t* sel_i, const float* sel_f, const double* boxes,
                                        const int32_t* inside, const int32_t* paths, float* targets, int64_t n_rows, int64_t* offsets, void* stream) {
    const PolyTables p = {nullptr, nullptr, 0, 0, const_cast<double*>(boxes), const_cast<int*>(inside), const_cast<int*>(paths), n_rows};
    const PasteTables c = {paste, n_paste, const_cast<int*>(sel_i), const_cast<float*>(sel_f)};
    return launch_targets("y3_augment_targets_paste", target_args(labels, label_offsets, images, n_images, items, count, S, S, targets, n_rows, offsets), &p, &c, stream);
}

extern "C" int y3_augment_polygons(const float* vertices, int64_t n_vertices, const int64_t* vertex_offsets, int64_t n_label_rows, const int64_t* label_offsets,
                                   const y3_dataset_image* images, int64_t n_images, const y3_augment_item* items, int32_t count, int32_t S, double* boxes, int32_t* inside,
                                   int32_t* paths, int64_t n_rows, void* stream) {
    return launch_polygons("y3_augment_polygons", target_args(nullptr, label_offsets, images, n_images, items, count, S, S),
                           {vertices, (const long long*)vertex_offsets, n_vertices, n_label_rows, boxes, inside, paths, n_rows}, nullptr, stream);
}

extern "C" int y3_augment_polygons_paste(const float* vertices, int64_t n_vertices, const int64_t* vertex_offsets, int64_t n_label_rows, const int64_t* label_offsets,
                                         const y3_dataset_image* images, int64_t n_images, const y3_augment_item* items, int32_t count, int32_t S, const int32_t* paste,
                                         int32_t n_paste, const int32_t* sel_i, const float* sel_f, double* boxes, int32_t* inside, int32_t* paths, int64_t n_rows, void* stream) {
    const PasteTables c = {paste, n_paste, const_cast<int*>(sel_i), const_cast<float*>(sel_f)};
    return launch_polygons("y3_augment_polygons_paste", target_args(nullptr, label_offsets, images, n_images, items, count, S, S),
                           {vertices, (const long long*)vertex_offsets, n_vertices, n_label_rows, boxes, inside, paths, n_rows}, &c, stream);
}

extern "C" int y3_augment_copy_paste_select(const float* labels, const int64_t* label_offsets, const int64_t* vertex_offsets, int64_t n_vertices, int64_t n_label_rows,
                                            const y3_dataset_image* images, int64_t n_images, const y3_augment_item* items, int32_t count, int32_t S, const int32_t* paste,
                                            int32_t n_paste, int32_t* sel_i, float* sel_f, void* stream) {
    const char* fn = "y3_augment_copy_paste_select";
    const TargetArgs a = target_args(labels, label_offsets, images, n_images, items, count, S, S);
    const PolyTables p = {nullptr, (const long long*)vertex_offsets, n_vertices, n_label_rows};
    const PasteTables c = {paste, n_paste, const_cast<int*>(sel_i), const_cast<float*>(sel_f)};
    if (!labels || !label_offsets || !vertex_offsets) Y3_FAIL("%s: null argument", fn);
    if (check_set(fn, a, &c)) return -1;
    if (bad_vertex_table(p)) Y3_FAIL("%s: bad geometry (%lld vertices, %lld label rows)", fn, p.n_verts, p.n_vert_rows);
    if (!aligned(label_offsets, 8) || !aligned(vertex_offsets, 8) || !aligned(labels, 4)) Y3_FAIL("%s: the offsets must be 8-byte, the label table 4-byte aligned", fn);
    if (count == 0) return 0;
    hipLaunchKernelGGL(copy_paste_select_kernel, dim3((unsigned)count * 2), dim3(BT), 0, (hipStream_t)stream, a, p, c);
    Y3_CHECK_LAUNCH();
    return 0;
}

extern "C" int y3_augment_copy_paste_raster(const float* vertices, int64_t n_vertices, const int64_t* vertex_offsets, int64_t n_label_rows, const int64_t* label_offsets,
                                            const y3_dataset_image* images, int64_t n_images, const y3_augment_item* items, int32_t count, int32_t S, const int32_t* paste,
                                            int32_t n_paste, const int32_t* sel_i, int32_t* masks, int32_t n_masks, void* stream) {
    const char* fn = "y3_augment_copy_paste_raster";
    const TargetArgs a = target_args(nullptr, label_offsets, images, n_images, items, count, S, S);
    const PolyTables p = {vertices, (const long long*)vertex_offsets, n_vertices, n_label_rows};
    const PasteTables c = {paste, n_paste, const_cast<int*>(sel_i), nullptr, (unsigned*)masks, n_masks};
    if (!vertices || !vertex_offsets || !label_offsets || !masks) Y3_FAIL("%s: null argument", fn);
    if (check_set(fn, a, &c, SEL_I_ONLY)) return -1;
    if (bad_vertex_table(p, 1) || n_masks < 1 || n_masks > 2 * count) Y3_FAIL("%s: bad geometry (%lld vertices, %lld label rows, %d masks for %d items)", fn, p.n_verts, p.n_vert_rows, n_masks, count);
    if (!aligned(label_offsets, 8) || !aligned(vertex_offsets, 8) || !aligned(vertices, 4) || !aligned(masks, 4)) Y3_FAIL("%s: the offsets must be 8-byte, the vertices and the masks 4-byte aligned", fn);
    hipLaunchKernelGGL(copy_paste_raster_kernel, dim3((unsigned)n_paste), dim3(BT), 0, (hipStream_t)stream, a, p, c);
    Y3_CHECK_LAUNCH();
    return 0;
}

