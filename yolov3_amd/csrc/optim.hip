// Fused optimizer step for gfx950: GradScaler.unscale_ + inf/nan check, clip_grad_norm_ (global L2), SGD with Nesterov
// momentum and per-tensor weight decay / lr, and the ModelEMA lerp -- two launches for the whole model instead of the
// reference's ~5 full passes over 248 MB and hundreds of foreach launches (reference train.py:414-422,
// utils/torch_utils.py:207-237 smart_optimizer, upstream ModelEMA.update).  HBM-bound streaming: one read of grad,
// read+write of param, momentum buffer and EMA.  No host synchronisation: the clip coefficient and the found-inf flag
// stay on the device (a step with inf/nan gradients is skipped, like GradScaler.step).
#include "y3_common.h"

namespace {

constexpr int CHUNK = 16384;  // elements per block

struct OptTensor {            // one entry per parameter tensor, DEVICE memory, built by the host mirror
    float* param;
    const float* grad;
    float* mom;               // momentum buffer (zero-initialised before the first step)
    float* ema;               // may be null
    long long numel;
    float lr, weight_decay;
    int first_chunk;          // prefix sum of chunk counts
    int pad;
};

// the moment optimizers' record (Adam / AdamW: s1 = exp_avg, s2 = exp_avg_sq, h0 = beta1, h1 = beta2; RMSProp: s1 = square_avg, s2 = momentum buffer or null,
// h0 = alpha, h1 = momentum).  Hyper-parameters are doubles, as torch holds them: 1 - beta2 = 0.001 taken from a float beta2 is already 6e-5 off.
struct MomentTensor {
    float* param;
    const float* grad;
    float* s1;
    float* s2;
    float* ema;               // may be null
    long long numel;
    double lr, weight_decay, h0, h1, eps;
    int first_chunk;          // prefix sum of chunk counts
    int pad;
};

template <class Rec>
__device__ int find_tensor(const Rec* __restrict__ t, int n, int chunk) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (t[mid].first_chunk <= chunk) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// pass 1: sum of squares of the (unscaled) gradients + non-finite detection; one partial per block
template <class Rec>
__global__ __launch_bounds__(256) void grad_norm_kernel(const Rec* __restrict__ t, int n, float inv_scale, const float* __restrict__ scale_dev,
                                                          float* __restrict__ partial, int* __restrict__ found_inf) {
    __shared__ float red[256];
    if (scale_dev) inv_scale *= 1.0f / scale_dev[0];   // dynamic loss scale (GradScaler): lives on the device, no host round trip
    const int ti = find_tensor(t, n, blockIdx.x);
    const Rec T = t[ti];
    const long long base = (long long)(blockIdx.x - T.first_chunk) * CHUNK;
    float a = 0.0f;
    bool bad = false;
    for (int i = threadIdx.x; i < CHUNK; i += 256) {
        const long long e = base + i;
        if (e < T.numel) {
            const float g = T.grad[e] * inv_scale;
            bad |= !(fabsf(g) <= 3.402823466e38f);
            a += g * g;
        }
    }
    red[threadIdx.x] = a;
    if (bad) *found_inf = 1;
    __syncthreads();
    for (int s = 128; s >= 1; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[blockIdx.x] = red[0];
}

// total norm (fixed-order sum of the partials) -> clip coefficient  min(1, max_norm / (norm + 1e-6))
__global__ __launch_bounds__(256) void clip_coef_kernel(const float* __restrict__ partial, int nchunks, float max_norm, float* __restrict__ out /* [norm, coef] */) {
    __shared__ double red[256];
    double a = 0.0;
    for (int i = threadIdx.x; i < nchunks; i += 256) a += (double)partial[i];
    red[threadIdx.x] = a;
    __syncthreads();
    for (int s = 128; s >= 1; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const float norm = (float)sqrt(red[0]);
        out[0] = norm;
        float c = max_norm > 0.0f ? max_norm / (norm + 1e-6f) : 1.0f;
        out[1] = c < 1.0f ? c : 1.0f;
    }
}

// The ModelEMA lerp (upstream ModelEMA.update: v *= d; v += (1 - d) * p), the ONE definition every kernel of this file applies: the fused steps to the parameters
// they just wrote, ema_update_kernel to everything else.  This file is built without FMA contraction: two products and a sum, each rounded once.
__device__ __forceinline__ float ema_lerp(float e, float p, float d) { return d * e + (1.0f - d) * p; }

// pass 2: p, buf, ema update (torch.optim.SGD semantics: g += wd*p; buf = first ? g : mu*buf + g; g = nesterov ? g + mu*buf : buf)
__global__ __launch_bounds__(256) void sgd_update_kernel(const OptTensor* __restrict__ t, int n, float inv_scale, const float* __restrict__ scale_dev,
                                                           const float* __restrict__ clip, const int* __restrict__ found_inf, float momentum, int nesterov, int first_step,
                                                           float ema_decay) {
    if (*found_inf) return;  // GradScaler.step skips the update when any gradient is inf/nan
    if (scale_dev) inv_scale *= 1.0f / scale_dev[0];
    const int ti = find_tensor(t, n, blockIdx.x);
    const OptTensor T = t[ti];
    const long long base = (long long)(blockIdx.x - T.first_chunk) * CHUNK;
    const float gs = inv_scale * clip[1];
    for (int i = threadIdx.x; i < CHUNK; i += 256) {
        const long long e = base + i;
        if (e >= T.numel) break;
        float p = T.param[e];
        float g = T.grad[e] * gs;
        if (T.weight_decay != 0.0f) g += T.weight_decay * p;
        float b = first_step ? g : momentum * T.mom[e] + g;
        T.mom[e] = b;
        g = nesterov ? g + momentum * b : b;
        p -= T.lr * g;
        T.param[e] = p;
        if (T.ema) T.ema[e] = ema_lerp(T.ema[e], p, ema_decay);
    }
}

// ---- Adam / AdamW / RMSProp: torch's single-tensor algorithms (torch/optim/adam.py, rmsprop.py; amsgrad, maximize, centered off), fp32 state --------------
// The step count t lives on the device: it advances only when the step is not skipped, so the bias corrections stay torch's after an overflow step.
__global__ void step_advance_kernel(int* __restrict__ step, const int* __restrict__ found_inf) {
    if (threadIdx.x == 0 && blockIdx.x == 0 && !*found_inf) *step = *step + 1;
}

// Tensor.lerp_(end, w) as ATen computes it
__device__ __forceinline__ float lerp_aten(float a, float b, float w) { return w < 0.5f ? a + w * (b - a) : b - (b - a) * (1.0f - w); }

struct AdamCoef {             // block-uniform, from the record and t
    float wd, decay, w1, b2, w2, bc2_sqrt, eps, neg_step;
    int decoupled;
    __device__ AdamCoef(const MomentTensor& T, int t, int decoupled_) : decoupled(decoupled_) {
        wd = (float)T.weight_decay;
        decay = (float)(1.0 - T.lr * T.weight_decay);
        w1 = (float)(1.0 - T.h0);
        b2 = (float)T.h1;
        w2 = (float)(1.0 - T.h1);
        const double bc1 = 1.0 - pow(T.h0, (double)t), bc2 = 1.0 - pow(T.h1, (double)t);
        bc2_sqrt = (float)sqrt(bc2);
        eps = (float)T.eps;
        neg_step = (float)(-(T.lr / bc1));
    }
    // g arrives unscaled and clipped; s1 = exp_avg, s2 = exp_avg_sq
    __device__ __forceinline__ void apply(float& p, float g, float& m, float& v) const {
        if (wd != 0.0f) {
            if (decoupled) p *= decay; else g += wd * p;
        }
        m = lerp_aten(m, g, w1);
        v = v * b2 + w2 * g * g;
        const float denom = sqrtf(v) / bc2_sqrt + eps;
        p += neg_step * m / denom;
    }
};

struct RmsCoef {
    float wd, alpha, w, eps, mu, neg_lr;
    __device__ RmsCoef(const MomentTensor& T, int, int) {
        wd = (float)T.weight_decay;
        alpha = (float)T.h0;
        w = (float)(1.0 - T.h0);
        eps = (float)T.eps;
        mu = (float)T.h1;
        neg_lr = (float)(-T.lr);
    }
    // s1 = square_avg, s2 = momentum buffer (read and written only when mu > 0)
    __device__ __forceinline__ void apply(float& p, float g, float& s, float& b) const {
        if (wd != 0.0f) g += wd * p;
        s = s * alpha + w * g * g;
        const float avg = sqrtf(s) + eps;
        if (mu > 0.0f) {
            b = b * mu + g / avg;
            p += neg_lr * b;
        } else {
            p += neg_lr * g / avg;
        }
    }
};

// pass 2 of the moment optimizers.  HBM-bound: per element one read of grad, read + write of param, the state buffers and EMA.  A tensor whose pointers are all
// 16-byte aligned is streamed as float4 (a chunk starts at a multiple of 16384 elements, so alignment carries over); the last numel % 4 elements and misaligned
// tensors (a gradient is a view into a flat arena: 4-byte alignment is all a record promises) go one float at a time.  HAS_S2 = false: RMSProp without momentum.
template <class Coef, bool HAS_S2>
__device__ __forceinline__ void moment_update_chunk(const MomentTensor& T, const Coef& c, long long base, float gs, float ema_decay) {
    const long long left = T.numel - base;
    const int lim = left < CHUNK ? (int)left : CHUNK;
    uintptr_t bits = (uintptr_t)T.param | (uintptr_t)T.grad | (uintptr_t)T.s1 | (uintptr_t)T.ema;
    if (HAS_S2) bits |= (uintptr_t)T.s2;
    const int nvec = (bits & 15) == 0 ? (lim & ~3) : 0;   // elements handled as float4
    for (int i = threadIdx.x * 4; i < nvec; i += 1024) {
        const long long e = base + i;
        f32x4 p = *(const f32x4*)(T.param + e);
        const f32x4 g = *(const f32x4*)(T.grad + e) * gs;
        f32x4 a = *(const f32x4*)(T.s1 + e);
        f32x4 b = {0.0f, 0.0f, 0.0f, 0.0f};
        if (HAS_S2) b = *(const f32x4*)(T.s2 + e);
        f32x4 m = {0.0f, 0.0f, 0.0f, 0.0f};
        if (T.ema) m = *(const f32x4*)(T.ema + e);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float pk = p[k], ak = a[k], bk = b[k];
            c.apply(pk, g[k], ak, bk);
            p[k] = pk, a[k] = ak, b[k] = bk;
        }
        *(f32x4*)(T.param + e) = p;
        *(f32x4*)(T.s1 + e) = a;
        if (HAS_S2) *(f32x4*)(T.s2 + e) = b;
        if (T.ema) {
#pragma unroll
            for (int k = 0; k < 4; ++k) m[k] = ema_lerp(m[k], p[k], ema_decay);
            *(f32x4*)(T.ema + e) = m;
        }
    }
    for (int i = nvec + threadIdx.x; i < lim; i += 256) {
        const long long e = base + i;
        float p = T.param[e], a = T.s1[e], b = HAS_S2 ? T.s2[e] : 0.0f;
        c.apply(p, T.grad[e] * gs, a, b);
        T.param[e] = p;
        T.s1[e] = a;
        if (HAS_S2) T.s2[e] = b;
        if (T.ema) T.ema[e] = ema_lerp(T.ema[e], p, ema_decay);
    }
}

template <class Coef>
__global__ __launch_bounds__(256) void moment_update_kernel(const MomentTensor* __restrict__ t, int n, float inv_scale, const float* __restrict__ scale_dev,
                                                              const float* __restrict__ clip, const int* __restrict__ found_inf, const int* __restrict__ step, int decoupled,
                                                              float ema_decay) {
    if (*found_inf) return;  // skipped step: parameters, state and EMA stay bit for bit
    if (scale_dev) inv_scale *= 1.0f / scale_dev[0];
    const int ti = find_tensor(t, n, blockIdx.x);
    const MomentTensor T = t[ti];
    const long long base = (long long)(blockIdx.x - T.first_chunk) * CHUNK;
    const float gs = inv_scale * clip[1];
    const Coef c(T, *step, decoupled);
    if (T.s2) moment_update_chunk<Coef, true>(T, c, base, gs, ema_decay);
    else moment_update_chunk<Coef, false>(T, c, base, gs, ema_decay);
}

// ModelEMA.update(model) on its own (reference train.py:421 after `scaler.step(optimizer)`; also what a fused step leaves over: the float buffers and the parameters
// it did not touch): ema = ema_lerp(ema, src, d) for every record, one launch.  Streams 12 bytes per element; float4 where both pointers allow it.
struct EmaTensor {
    float* ema;
    const float* src;
    long long numel;
    int first_chunk;          // prefix sum of chunk counts
    int pad;
};
static_assert(sizeof(EmaTensor) == 32, "the host mirror (yolov3_amd/optim.py) packs 32-byte records");

// ModelEMA's counter and decay ON THE DEVICE (y3_ema_update_counted): a fused optimizer step learns only on the device whether it was skipped (found_inf), and the
// reference's d = decay * (1 - exp(-updates / tau)) depends on how many updates were really made.  The host mirror (yolov3_amd/optim.py) packs these 24 bytes.
struct EmaState {
    int updates;
    float d;                  // the decay of update number `updates`
    double decay, tau;
};
static_assert(sizeof(EmaState) == 24, "the host mirror (yolov3_amd/optim.py) packs 24 bytes");

// updates += 1 and the decay that goes with it (in double, rounded once to fp32: what the host computes for y3_ema_update) -- unless the step was skipped
__global__ void ema_advance_kernel(EmaState* __restrict__ s, const int* __restrict__ found_inf) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    if (found_inf && *found_inf) return;
    const int n = s->updates + 1;
    s->updates = n;
    s->d = (float)(s->decay * (1.0 - exp(-(double)n / s->tau)));
}

// `state` given: the decay is state->d; `found_inf` given and set: nothing is written (a skipped step leaves the averages bit for bit)
__global__ __launch_bounds__(256) void ema_update_kernel(const EmaTensor* __restrict__ t, int n, float d, const EmaState* __restrict__ state,
                                                           const int* __restrict__ found_inf) {
    if (found_inf && *found_inf) return;
    if (state) d = state->d;
    const int ti = find_tensor(t, n, blockIdx.x);
    const EmaTensor T = t[ti];
    const long long base = (long long)(blockIdx.x - T.first_chunk) * CHUNK;
    const long long left = T.numel - base;
    const int lim = left < CHUNK ? (int)left : CHUNK;
    const int nvec = (((uintptr_t)T.ema | (uintptr_t)T.src) & 15) == 0 ? (lim & ~3) : 0;
    for (int i = threadIdx.x * 4; i < nvec; i += 1024) {
        const long long e = base + i;
        f32x4 m = *(const f32x4*)(T.ema + e);
        const f32x4 p = *(const f32x4*)(T.src + e);
#pragma unroll
        for (int k = 0; k < 4; ++k) m[k] = ema_lerp(m[k], p[k], d);
        *(f32x4*)(T.ema + e) = m;
    }
    for (int i = nvec + threadIdx.x; i < lim; i += 256) {
        const long long e = base + i;
        T.ema[e] = ema_lerp(T.ema[e], T.src[e], d);
    }
}

// torch.cuda.amp.GradScaler.update() (reference train.py:345,416-417; ATen _amp_update_scale_): on a step that found inf/nan the scale
// is multiplied by backoff_factor and the growth counter reset; otherwise the counter advances and every growth_interval clean steps
// the scale is multiplied by growth_factor (unless that overflows fp32).  All on the device.
__global__ void loss_scale_update_kernel(float* __restrict__ scale, int* __restrict__ growth_tracker, const int* __restrict__ found_inf, float growth_factor,
                                         float backoff_factor, int growth_interval) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    if (*found_inf) {
        *scale = *scale * backoff_factor;
        *growth_tracker = 0;
    } else {
        const int successful = *growth_tracker + 1;
        if (successful == growth_interval) {
            const float grown = *scale * growth_factor;
            if (fabsf(grown) <= 3.402823466e38f) *scale = grown;
            *growth_tracker = 0;
        } else {
            *growth_tracker = successful;
        }
    }
}

// the owner's step of the two-phase gradient exchange (parallel.GradBuckets, exchange = "direct"): out[i] = (parts[0][i] + parts[1][i] + ... + parts[P-1][i]) * scale,
// the P contributions added in rank order (every rank receives this one sum: replicas stay bit-identical), one pass, one launch
__global__ __launch_bounds__(256) void shard_mean_kernel(const float* __restrict__ parts, int P, long long n, float scale, float* __restrict__ out) {
    const long long i = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i >= n) return;
    if (i + 4 <= n && (((uintptr_t)parts | (uintptr_t)out) & 15) == 0 && (n & 3) == 0) {
        f32x4 a = *(const f32x4*)(parts + i);
        for (int r = 1; r < P; ++r) a += *(const f32x4*)(parts + (long long)r * n + i);
        *(f32x4*)(out + i) = a * scale;
        return;
    }
    for (long long j = i; j < n && j < i + 4; ++j) {
        float a = parts[j];
        for (int r = 1; r < P; ++r) a += parts[(long long)r * n + j];
        out[j] = a * scale;
    }
}

}  // namespace

extern "C" int y3_shard_mean(const float* parts, int32_t n_parts, int64_t n, float scale, float* out, void* stream) {
    if (!parts || !out || n_parts < 1 || n < 0) Y3_FAIL("y3_shard_mean: bad argument");
    if (n == 0) return 0;
    hipLaunchKernelGGL(shard_mean_kernel, dim3((unsigned)((n + 1023) / 1024)), dim3(256), 0, (hipStream_t)stream, parts, n_parts, (long long)n, scale, out);
    Y3_CHECK_LAUNCH();
    return 0;
}

extern "C" size_t y3_sgd_tensor_record_bytes(void) { return sizeof(OptTensor); }

static int sgd_step_impl(const void* tensor_table, int32_t n_tensors, int32_t n_chunks, float inv_scale, const float* scale_dev, float max_norm, float momentum,
                         int32_t nesterov, int32_t first_step, float ema_decay, float* scratch, int32_t* found_inf, void* stream) {
    if (!tensor_table || !scratch || !found_inf || n_tensors <= 0 || n_chunks <= 0) Y3_FAIL("y3_sgd_step: bad argument");
    hipStream_t st = (hipStream_t)stream;
    const OptTensor* t = (const OptTensor*)tensor_table;
    Y3_HIP(hipMemsetAsync(found_inf, 0, sizeof(int), st));
    hipLaunchKernelGGL(grad_norm_kernel<OptTensor>, dim3((unsigned)n_chunks), dim3(256), 0, st, t, n_tensors, inv_scale, scale_dev, scratch + 2, found_inf);
    Y3_CHECK_LAUNCH();
    hipLaunchKernelGGL(clip_coef_kernel, dim3(1), dim3(256), 0, st, (const float*)(scratch + 2), n_chunks, max_norm, scratch);
    Y3_CHECK_LAUNCH();
    hipLaunchKernelGGL(sgd_update_kernel, dim3((unsigned)n_chunks), dim3(256), 0, st, t, n_tensors, inv_scale, scale_dev, (const float*)scratch, (const int*)found_inf, momentum,
                       nesterov, first_step, ema_decay);
    Y3_CHECK_LAUNCH();
    return 0;
}

extern "C" int y3_sgd_step(const void* tensor_table, int32_t n_tensors, int32_t n_chunks, float inv_scale, float max_norm, float momentum, int32_t nesterov,
                           int32_t first_step, float ema_decay, float* scratch /* n_chunks + 2 floats */, int32_t* found_inf, void* stream) {
    return sgd_step_impl(tensor_table, n_tensors, n_chunks, inv_scale, nullptr, max_norm, momentum, nesterov, first_step, ema_decay, scratch, found_inf, stream);
}

extern "C" int y3_sgd_step_dynamic(const void* tensor_table, int32_t n_tensors, int32_t n_chunks, const float* loss_scale, float max_norm, float momentum, int32_t nesterov,
                                   int32_t first_step, float ema_decay, float* scratch, int32_t* found_inf, void* stream) {
    if (!loss_scale) Y3_FAIL("y3_sgd_step_dynamic: null loss scale");
    return sgd_step_impl(tensor_table, n_tensors, n_chunks, 1.0f, loss_scale, max_norm, momentum, nesterov, first_step, ema_decay, scratch, found_inf, stream);
}

extern "C" int y3_loss_scale_update(float* loss_scale, int32_t* growth_tracker, const int32_t* found_inf, float growth_factor, float backoff_factor, int32_t growth_interval,
                                    void* stream) {
    if (!loss_scale || !growth_tracker || !found_inf || growth_interval < 1) Y3_FAIL("y3_loss_scale_update: bad argument");
    hipLaunchKernelGGL(loss_scale_update_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, loss_scale, growth_tracker, found_inf, growth_factor, backoff_factor, growth_interval);
    Y3_CHECK_LAUNCH();
    return 0;
}

extern "C" int y3_ema_update(const void* tensor_table, int32_t n_tensors, int32_t n_chunks, float d, void* stream) {
    if (!tensor_table) Y3_FAIL("y3_ema_update: null tensor table");
    if (n_tensors <= 0 || n_chunks <= 0) Y3_FAIL("y3_ema_update: n_tensors %d and n_chunks %d must be positive", (int)n_tensors, (int)n_chunks);
    if (!(d >= 0.0f && d <= 1.0f)) Y3_FAIL("y3_ema_update: decay %g is outside [0, 1]", (double)d);
    hipLaunchKernelGGL(ema_update_kernel, dim3((unsigned)n_chunks), dim3(256), 0, (hipStream_t)stream, (const EmaTensor*)tensor_table, n_tensors, d, (const EmaState*)nullptr,
                       (const int*)nullptr);
    Y3_CHECK_LAUNCH();
    return 0;
}

extern "C" int y3_ema_update_counted(const void* tensor_table, int32_t n_tensors, int32_t n_chunks, void* ema_state, const int32_t* found_inf, void* stream) {
    if (!tensor_table) Y3_FAIL("y3_ema_update_counted: null tensor table");
    if (n_tensors <= 0 || n_chunks <= 0) Y3_FAIL("y3_ema_update_counted: n_tensors %d and n_chunks %d must be positive", (int)n_tensors, (int)n_chunks);
    if (!ema_state) Y3_FAIL("y3_ema_update_counted: null ema state");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(ema_advance_kernel, dim3(1), dim3(64), 0, st, (EmaState*)ema_state, (const int*)found_inf);
    Y3_CHECK_LAUNCH();
    hipLaunchKernelGGL(ema_update_kernel, dim3((unsigned)n_chunks), dim3(256), 0, st, (const EmaTensor*)tensor_table, n_tensors, 0.0f, (const EmaState*)ema_state,
                       (const int*)found_inf);
    Y3_CHECK_LAUNCH();
    return 0;
}

extern "C" size_t y3_optim_tensor_record_bytes(void) { return sizeof(MomentTensor); }

template <class Coef>
static int moment_step_impl(const char* who, const void* tensor_table, int32_t n_tensors, int32_t n_chunks, float inv_scale, const float* scale_dev, float max_norm, int32_t decoupled,
                            float ema_decay, int32_t* step, float* scratch, int32_t* found_inf, void* stream) {
    if (!tensor_table) Y3_FAIL("%s: null tensor table", who);
    if (n_tensors <= 0 || n_chunks <= 0) Y3_FAIL("%s: n_tensors %d and n_chunks %d must be positive", who, (int)n_tensors, (int)n_chunks);
    if (!step) Y3_FAIL("%s: null step counter", who);
    if (!scratch || !found_inf) Y3_FAIL("%s: null scratch or found_inf", who);
    hipStream_t st = (hipStream_t)stream;
    const MomentTensor* t = (const MomentTensor*)tensor_table;
    Y3_HIP(hipMemsetAsync(found_inf, 0, sizeof(int), st));
    hipLaunchKernelGGL(grad_norm_kernel<MomentTensor>, dim3((unsigned)n_chunks), dim3(256), 0, st, t, n_tensors, inv_scale, scale_dev, scratch + 2, found_inf);
    Y3_CHECK_LAUNCH();
    hipLaunchKernelGGL(clip_coef_kernel, dim3(1), dim3(256), 0, st, (const float*)(scratch + 2), n_chunks, max_norm, scratch);
    Y3_CHECK_LAUNCH();
    hipLaunchKernelGGL(step_advance_kernel, dim3(1), dim3(64), 0, st, step, (const int*)found_inf);
    Y3_CHECK_LAUNCH();
    hipLaunchKernelGGL(moment_update_kernel<Coef>, dim3((unsigned)n_chunks), dim3(256), 0, st, t, n_tensors, inv_scale, scale_dev, (const float*)scratch, (const int*)found_inf,
                       (const int*)step, decoupled, ema_decay);
    Y3_CHECK_LAUNCH();
    return 0;
}

extern "C" int y3_adam_step(const void* tensor_table, int32_t n_tensors, int32_t n_chunks, float inv_scale, const float* loss_scale, float max_norm, int32_t decoupled,
                            float ema_decay, int32_t* step, float* scratch, int32_t* found_inf, void* stream) {
    return moment_step_impl<AdamCoef>("y3_adam_step", tensor_table, n_tensors, n_chunks, inv_scale, loss_scale, max_norm, decoupled, ema_decay, step, scratch, found_inf, stream);
}

extern "C" int y3_rmsprop_step(const void* tensor_table, int32_t n_tensors, int32_t n_chunks, float inv_scale, const float* loss_scale, float max_norm, float ema_decay,
                               int32_t* step, float* scratch, int32_t* found_inf, void* stream) {
    return moment_step_impl<RmsCoef>("y3_rmsprop_step", tensor_table, n_tensors, n_chunks, inv_scale, loss_scale, max_norm, 0, ema_decay, step, scratch, found_inf, stream);
}
