// The batch's way from the loader to model(imgs) in the reference's train loop, on gfx950:
//   * y3_resize_bilinear   train.py:380 + 394-399: `imgs.float() / 255` and the --multi-scale F.interpolate(size=ns, mode="bilinear", align_corners=False)
//     in one pass over the uint8 batch -- no fp32 copy of the batch goes to memory and comes back;
//   * y3_quad_collate_u8   utils/dataloaders.py:833-858 (collate_fn4, --quad): every group of four images becomes either the bilinear x2 upsample of its first
//     image or the 2x2 tile of all four, in one launch.
// fp32 arithmetic in torch's operation order (built with -ffp-contract=off; `/` is the IEEE division of torch's CPU kernels); the coordinate and weight
// arithmetic is y3_bilinear.h's, shared with y3_scale_img.
#include "y3_bilinear.h"
#include "y3_common.h"

namespace {

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// 8 consecutive outputs of one row: 16 bytes per store (two stores for fp32); d is 16-byte aligned
template <typename D> Y3_DEV void store8(D* d, const float (&v)[8]) {
    u32x4 q = {pack2<D>(v[0], v[1]), pack2<D>(v[2], v[3]), pack2<D>(v[4], v[5]), pack2<D>(v[6], v[7])};
    *reinterpret_cast<u32x4*>(d) = q;
}
template <> Y3_DEV void store8<float>(float* d, const float (&v)[8]) {
    const f32x4 lo = {v[0], v[1], v[2], v[3]}, hi = {v[4], v[5], v[6], v[7]};
    reinterpret_cast<f32x4*>(d)[0] = lo;
    reinterpret_cast<f32x4*>(d)[1] = hi;
}

struct ResizeArgs {
    const void* src;
    void* dst;
    int planes, h, w, oh, ow, spr, segs;   // spr = ceil(ow / 64) 64-wide segments per output row, segs = oh * spr
    float rh, rw, divisor;
};
constexpr int RS_K = 8;   // segments per wave and pass
// The output rows are cut into 64-wide segments; a wave takes RS_K consecutive segments (they may run over a row's end into the next row), lane l computing column
// 64 s + l of each: consecutive lanes read consecutive source pixels, every tap load of a wave falls into one or two cache lines.  A lane's x taps and weights
// (the y ones are uniform over a wave) are computed once and serve every plane it visits (grid z strides the planes, grid x the tiles of 4 x RS_K segments).
// VEC (ow % 8 == 0, dst 16-byte aligned): the wave's 512 results cross lanes through LDS, so that every lane stores 8 consecutive columns, 16 bytes (two
// stores for fp32); otherwise every lane stores its own elements under the row's bound.  Columns past the row's end and segments past the last one clamp their
// taps to the last column / segment: in bounds, never stored.  A uint8 source takes value / divisor from a 256-entry table: the same IEEE quotient, once per block.
template <typename S, typename D, bool VEC> __global__ __launch_bounds__(256) void resize_bilinear_kernel(const ResizeArgs a) {
    constexpr bool U8 = sizeof(S) == 1;
    __shared__ float lut[U8 ? 256 : 1];
    __shared__ float stage[VEC ? 2 : 1][4][VEC ? RS_K * 64 : 1];   // two buffers: one barrier per pass
    if constexpr (U8) {
        lut[threadIdx.x] = (float)threadIdx.x / a.divisor;
        __syncthreads();
    }
    const S* src = (const S*)a.src;
    D* dst = (D*)a.dst;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const long long hw = (long long)a.h * a.w, ohw = (long long)a.oh * a.ow;
    const bool divide = !U8 && a.divisor != 1.0f;   // x / 1 is x: the floating-point batches of train.py:399 skip the division
    const int tiles = (a.segs + 4 * RS_K - 1) / (4 * RS_K);
    int buf = 0;
    for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int seg0 = (tile * 4 + wave) * RS_K;
        int y0[RS_K], y1[RS_K], x0[RS_K], x1[RS_K], o[RS_K];
        float ly[RS_K], lx[RS_K];
        bool ok[RS_K];
#pragma unroll
        for (int k = 0; k < RS_K; ++k) {
            const int seg = min(seg0 + k, a.segs - 1), oy = seg / a.spr, ox = (seg - oy * a.spr) * 64 + lane;
            ok[k] = seg0 + k < a.segs && ox < a.ow;
            o[k] = oy * a.ow + ox;   // oh * ow fits int32 (checked by the caller)
            y3_bilinear_tap(a.rh, oy, a.h, y0[k], y1[k], ly[k]);
            y3_bilinear_tap(a.rw, min(ox, a.ow - 1), a.w, x0[k], x1[k], lx[k]);
        }
        // the 8 columns this lane stores (VEC): segment seg0 + lane / 8, columns 8 (lane % 8) .. + 7 of it
        const int rseg = min(seg0 + (lane >> 3), a.segs - 1), roy = rseg / a.spr, rox = (rseg - roy * a.spr) * 64 + (lane & 7) * 8;
        const bool rok = seg0 + (lane >> 3) < a.segs && rox < a.ow;
        const int ro = roy * a.ow + rox;
        for (int pl = blockIdx.z; pl < a.planes; pl += gridDim.z) {
            const S* s = src + pl * hw;
            float t[4][RS_K], v[RS_K];
            if constexpr (U8) {
                unsigned char b[4][RS_K];
#pragma unroll
                for (int k = 0; k < RS_K; ++k) {
                    const unsigned char* s0 = (const unsigned char*)s + (long long)y0[k] * a.w;
                    const unsigned char* s1 = (const unsigned char*)s + (long long)y1[k] * a.w;
                    b[0][k] = s0[x0[k]]; b[1][k] = s0[x1[k]]; b[2][k] = s1[x0[k]]; b[3][k] = s1[x1[k]];
                }
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int k = 0; k < RS_K; ++k) t[i][k] = lut[b[i][k]];   // each tap divided BEFORE the lerp: `imgs.float() / 255`, then the interpolate
            } else {
#pragma unroll
                for (int k = 0; k < RS_K; ++k) {
                    const S* s0 = s + (long long)y0[k] * a.w;
                    const S* s1 = s + (long long)y1[k] * a.w;
                    t[0][k] = to_f32<S>(s0[x0[k]]); t[1][k] = to_f32<S>(s0[x1[k]]); t[2][k] = to_f32<S>(s1[x0[k]]); t[3][k] = to_f32<S>(s1[x1[k]]);
                }
                if (divide) {
#pragma unroll
                    for (int i = 0; i < 4; ++i)
#pragma unroll
                        for (int k = 0; k < RS_K; ++k) t[i][k] = t[i][k] / a.divisor;
                }
            }
#pragma unroll
            for (int k = 0; k < RS_K; ++k) v[k] = y3_bilinear_mix(1.0f - ly[k], 1.0f - lx[k], ly[k], lx[k], t[0][k], t[1][k], t[2][k], t[3][k]);
            D* d = dst + pl * ohw;
            if constexpr (VEC) {
                float* st = stage[buf][wave];
#pragma unroll
                for (int k = 0; k < RS_K; ++k) st[k * 64 + lane] = v[k];
                __syncthreads();   // (uniform: both loops run the same trips in every thread of the block; the other buffer is rewritten only after the next barrier)
                if (rok) {
                    const f32x4 lo = *reinterpret_cast<const f32x4*>(st + lane * 8), hi = *reinterpret_cast<const f32x4*>(st + lane * 8 + 4);
                    const float r[8] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
                    store8<D>(d + ro, r);
                }
                buf ^= 1;
            } else {
#pragma unroll
                for (int k = 0; k < RS_K; ++k)
                    if (ok[k]) d[o[k]] = from_f32<D>(v[k]);
            }
        }
    }
}

template <typename S, typename D> void launch_resize(const ResizeArgs& a, bool vec, dim3 grid, hipStream_t st) {
    if (vec) hipLaunchKernelGGL((resize_bilinear_kernel<S, D, true>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((resize_bilinear_kernel<S, D, false>), grid, dim3(256), 0, st, a);
}
template <typename S> bool launch_resize_to(int dst_dtype, const ResizeArgs& a, bool vec, dim3 grid, hipStream_t st) {
    switch (dst_dtype) {
        case Y3_F32: launch_resize<S, float>(a, vec, grid, st); return true;
        case Y3_F16: launch_resize<S, f16_t>(a, vec, grid, st); return true;
        case Y3_BF16: launch_resize<S, bf16_t>(a, vec, grid, st); return true;
        default: return false;
    }
}

// the grid of both kernels: x over the per-plane items (capped, strided), z over the planes (capped, strided), about 2048 blocks in all
dim3 edge_grid(long long items, int planes) {
    long long gx = (items + 255) / 256;
    if (gx > 2048) gx = 2048;
    long long gz = 2048 / gx;
    if (gz > 64) gz = 64;
    if (gz > planes) gz = planes;
    if (gz < 1) gz = 1;
    return dim3((unsigned)gx, 1, (unsigned)gz);
}

struct QuadArgs {
    const unsigned char* src;
    const unsigned char* flags;
    unsigned char* dst;
    int planes, c, h, w, groups;   // planes = (bs / 4) * c output planes of (2h, 2w); groups = ceil(2w / 4): a lane owns 4 consecutive x of one output row
};
// One lane: 4 consecutive output bytes of a row, for every plane it visits.  The group's flag (uniform over the block: a block works on one plane at a time)
// selects the x2 upsample of image 4g -- torch maps coordinates with 1 / scale_factor = 0.5, every weight is 0.25 or 0.75 and every product and sum is exact in
// fp32; `.type(uint8)` truncates -- or the tile [[4g, 4g+2], [4g+1, 4g+3]].  VEC: w even and dst 4-byte aligned, one 4-byte store per group.
template <bool VEC> __global__ __launch_bounds__(256) void quad_collate_u8_kernel(const QuadArgs a) {
    const int H = 2 * a.h, W = 2 * a.w;
    const long long items = (long long)H * a.groups, hw = (long long)a.h * a.w;
    for (long long it = (long long)blockIdx.x * 256 + threadIdx.x; it < items; it += (long long)gridDim.x * 256) {
        const int oy = (int)it / a.groups, ox = ((int)it - oy * a.groups) * 4;
        int y0, y1, x0[4], x1[4], tx[4], right[4];
        float ly, lx[4];
        y3_bilinear_tap(0.5f, oy, a.h, y0, y1, ly);
        const int below = oy >= a.h ? 1 : 0, ty = oy - below * a.h;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int x = VEC ? ox + j : min(ox + j, W - 1);
            y3_bilinear_tap(0.5f, x, a.w, x0[j], x1[j], lx[j]);
            right[j] = x >= a.w ? 1 : 0;
            tx[j] = x - right[j] * a.w;
        }
        const float hy = 1.0f - ly;
        for (int pl = blockIdx.z; pl < a.planes; pl += gridDim.z) {
            const int g = pl / a.c, ch = pl - g * a.c;
            unsigned char v[4];
            if (a.flags[g]) {
                const unsigned char* s = a.src + ((long long)(4 * g) * a.c + ch) * hw;
                const unsigned char* s0 = s + (long long)y0 * a.w;
                const unsigned char* s1 = s + (long long)y1 * a.w;
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    v[j] = (unsigned char)y3_bilinear_mix(hy, 1.0f - lx[j], ly, lx[j], (float)s0[x0[j]], (float)s0[x1[j]], (float)s1[x0[j]], (float)s1[x1[j]]);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] = a.src[((long long)(4 * g + below + 2 * right[j]) * a.c + ch) * hw + (long long)ty * a.w + tx[j]];
            }
            unsigned char* d = a.dst + ((long long)pl * H + oy) * W + ox;
            if (VEC) {
                *reinterpret_cast<unsigned*>(d) = (unsigned)v[0] | ((unsigned)v[1] << 8) | ((unsigned)v[2] << 16) | ((unsigned)v[3] << 24);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (ox + j < W) d[j] = v[j];
            }
        }
    }
}

}  // namespace

extern "C" int y3_resize_bilinear(const void* src, int32_t src_dtype, int32_t n, int32_t c, int32_t h, int32_t w, void* dst, int32_t dst_dtype, int32_t oh, int32_t ow, float divisor,
                                  void* stream) {
    if (!src || !dst) Y3_FAIL("y3_resize_bilinear: null argument");
    if (n < 0 || c < 1 || h < 1 || w < 1 || oh < 1 || ow < 1) Y3_FAIL("y3_resize_bilinear: bad geometry (%dx%dx%dx%d -> %dx%d)", n, c, h, w, oh, ow);
    if (src_dtype != Y3_U8 && src_dtype != Y3_F32 && src_dtype != Y3_F16 && src_dtype != Y3_BF16) Y3_FAIL("y3_resize_bilinear: unsupported source dtype %d", src_dtype);
    if (dst_dtype != Y3_F32 && dst_dtype != Y3_F16 && dst_dtype != Y3_BF16) Y3_FAIL("y3_resize_bilinear: unsupported output dtype %d (float32 / float16 / bfloat16)", dst_dtype);
    if (!(divisor > 0.0f)) Y3_FAIL("y3_resize_bilinear: divisor %g must be positive", (double)divisor);
    if ((long long)n * c > 0x7fffffffLL) Y3_FAIL("y3_resize_bilinear: too many planes");
    if ((long long)h * w > 0x7fffffffLL || (long long)oh * ((long long)ow + 63) > 0x7fffffffLL) Y3_FAIL("y3_resize_bilinear: a plane of %dx%d -> %dx%d is too large", h, w, oh, ow);
    if (n == 0) return 0;
    ResizeArgs a;
    a.src = src; a.dst = dst; a.planes = n * c; a.h = h; a.w = w; a.oh = oh; a.ow = ow; a.spr = (ow + 63) / 64; a.segs = oh * a.spr;
    a.rh = (float)h / (float)oh;   // torch's area_pixel_compute_scale without a scale factor: input size / output size
    a.rw = (float)w / (float)ow;
    a.divisor = divisor;
    const bool vec = (ow % 8) == 0 && ((uintptr_t)dst % 16) == 0;
    const dim3 grid = edge_grid(((long long)a.segs + 4 * RS_K - 1) / (4 * RS_K) * 256, a.planes);
    bool ok = false;
    switch (src_dtype) {
        case Y3_U8: ok = launch_resize_to<unsigned char>(dst_dtype, a, vec, grid, (hipStream_t)stream); break;
        case Y3_F32: ok = launch_resize_to<float>(dst_dtype, a, vec, grid, (hipStream_t)stream); break;
        case Y3_F16: ok = launch_resize_to<f16_t>(dst_dtype, a, vec, grid, (hipStream_t)stream); break;
        case Y3_BF16: ok = launch_resize_to<bf16_t>(dst_dtype, a, vec, grid, (hipStream_t)stream); break;
    }
    if (!ok) Y3_FAIL("y3_resize_bilinear: unsupported dtype pair %d -> %d", src_dtype, dst_dtype);
    Y3_CHECK_LAUNCH();
    return 0;
}

extern "C" int y3_quad_collate_u8(const uint8_t* src, int32_t bs, int32_t c, int32_t h, int32_t w, const uint8_t* upsample_flags, uint8_t* dst, void* stream) {
    if (!src || !upsample_flags || !dst) Y3_FAIL("y3_quad_collate_u8: null argument");
    if (bs < 0 || c < 1 || h < 1 || w < 1) Y3_FAIL("y3_quad_collate_u8: bad geometry (%dx%dx%dx%d)", bs, c, h, w);
    if (bs % 4) Y3_FAIL("y3_quad_collate_u8: batch size %d is not a multiple of 4", bs);
    if ((long long)bs * c > 0x7fffffffLL) Y3_FAIL("y3_quad_collate_u8: too many planes");
    const int groups = (int)(((long long)w + 1) / 2);   // ceil(2w / 4)
    if ((long long)h * w > 0x1fffffffLL || 2LL * h * groups * 4 > 0x7fffffffLL) Y3_FAIL("y3_quad_collate_u8: a plane of %dx%d is too large", h, w);
    if (bs == 0) return 0;
    QuadArgs a;
    a.src = src; a.flags = upsample_flags; a.dst = dst; a.planes = bs / 4 * c; a.c = c; a.h = h; a.w = w; a.groups = groups;
    const dim3 grid = edge_grid(2LL * h * groups, a.planes);
    if ((w % 2) == 0 && ((uintptr_t)dst % 4) == 0) hipLaunchKernelGGL(quad_collate_u8_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(quad_collate_u8_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, a);
    Y3_CHECK_LAUNCH();
    return 0;
}
