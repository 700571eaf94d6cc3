// Fused AMSGrad over the flat trainable-parameter buffer + the non-finite-gradient guard of dynamic loss scaling, all fp32.
// torch.optim.Adam(amsgrad=True) semantics (run.py:134).  (The refresh of the 16-bit weight copies: norm_embed.hip.)
#include <algorithm>

#include "common.h"

namespace {

typedef __attribute__((ext_vector_type(4))) unsigned u32x4_t;

// guard (may be NULL): guard[0] = stamp of the last optimiser step whose gradient held a non-finite value, guard[1] = how many
// steps have been skipped for that so far (tnr_grad_nonfinite).  A launch stamped guard[0] leaves parameters and state untouched:
// the skipped step of dynamic loss scaling.  Adam's bias corrections depend on the number of steps actually TAKEN, which the host
// knows only with a lag: it passes the factors for step, step - 1, step - 2 and how many skips it has accounted for, the kernel
// picks by the skips it has not (all factors computed on the host, in double: the same bits as the unguarded launch).
// The learning rate may differ between the three candidates (a warmup / decay schedule follows the steps TAKEN, like the bias
// corrections): lr_c1[k] = lr_k / c1(t_k), and for the decay lr_wd[k] = lr_k * weight_decay.  lr_wd travels in a struct of its own
// BEHIND every other argument: inside AdamFactors it would move the arguments after it, and the instantiations without decay
// would no longer be, instruction for instruction, the kernels they were.
struct AdamFactors { float lr_c1[3], inv_sqrt_c2[3]; unsigned known_skips; };
struct AdamDecay { float lr_wd[3]; };
// The exponential moving average of the parameters (tnr_adamw_step_ema), behind AdamDecay for the same reason: e = the fp32 buffer
// of the averages, laid out like p (the same slice of it), w[k] = 1 - decay of candidate k (a warm-up of the decay follows the
// updates TAKEN, like the rates).
struct AdamEma { float* e; float w[3]; };
// CLIP: the gradient is scaled by gscale * clip[0], the coefficient grad_clip_commit_kernel left on the device (global-norm
// clipping); without it `clip` is never read and the kernel is the unclipped one.
// WD: decoupled weight decay in torch.optim.AdamW's order - p *= 1 - lr_k wd first, then the update on the undecayed gradient
// (the decay sees neither grad_scale nor the clip coefficient) - for the elements whose bit is set in `wbits`: one bit per
// element of the WHOLE flat buffer, bit (e & 31) of word e >> 5, this launch's slice starting at element `first` of it.  first and
// a thread's offset are multiples of 4, so its four bits are one nibble of one word.  Without WD neither wbits, first nor lr_wd is
// read and the kernel is the one without decay.  A launch stamped guard[0] decays nothing.
// EMA: once p_new is formed, e <- e + w_k (p_new - e) (one fma), e read and written like p: 16 bytes in the vector body, scalars
// in the tail; +8 bytes per element on 36 (AMSGrad) or 28 (Adam).  A launch stamped guard[0] returns before touching e.  Without
// EMA `a` is never read and the kernel is the one without the average.
template <bool AMS, bool CLIP, bool WD, bool EMA>
__global__ __launch_bounds__(256) void amsgrad_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                      float* __restrict__ m, float* __restrict__ v,
                                                      float* __restrict__ vmax, int64_t n, AdamFactors f,
                                                      float b1, float b2, float eps, float gscale,
                                                      const unsigned* __restrict__ guard, unsigned stamp,
                                                      const float* __restrict__ clip,
                                                      const unsigned* __restrict__ wbits, int64_t first, AdamDecay d,
                                                      AdamEma a) {
    if (CLIP) gscale *= clip[0];
    float lr_c1 = f.lr_c1[0], inv_sqrt_c2 = f.inv_sqrt_c2[0], keep = 1.f, w = 0.f;
    if (WD) keep = 1.f - d.lr_wd[0];
    if (EMA) w = a.w[0];
    if (guard) {
        if (guard[0] == stamp) return;
        const unsigned k = guard[1] - f.known_skips;
        if (k == 1) { lr_c1 = f.lr_c1[1]; inv_sqrt_c2 = f.inv_sqrt_c2[1]; if (WD) keep = 1.f - d.lr_wd[1]; if (EMA) w = a.w[1]; }
        else if (k >= 2) { lr_c1 = f.lr_c1[2]; inv_sqrt_c2 = f.inv_sqrt_c2[2]; if (WD) keep = 1.f - d.lr_wd[2]; if (EMA) w = a.w[2]; }
    }
    float* __restrict__ e = EMA ? a.e : nullptr;
    int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (i >= n) return;
    unsigned nib = 0;                       // bit r: element i + r decays (i < n, so the word lies inside the map)
    if (WD) nib = wbits[(first + i) >> 5] >> ((unsigned)(first + i) & 31u);
    if (i + 4 <= n) {
        f32x4 gv = *(const f32x4*)(g + i) * gscale;
        f32x4 mv = *(const f32x4*)(m + i) * b1 + (1.f - b1) * gv;
        f32x4 vv = *(const f32x4*)(v + i) * b2 + (1.f - b2) * gv * gv;
        f32x4 vm = vv;
        if (AMS) vm = *(const f32x4*)(vmax + i);
        f32x4 pv = *(const f32x4*)(p + i);
        f32x4 ev = pv;
        if (EMA) ev = *(const f32x4*)(e + i);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            if (AMS) vm[r] = fmaxf(vm[r], vv[r]);
            if (WD) pv[r] = (nib >> r) & 1u ? pv[r] * keep : pv[r];
            pv[r] -= lr_c1 * (mv[r] / (sqrtf(vm[r]) * inv_sqrt_c2 + eps));
            if (EMA) ev[r] = __builtin_fmaf(w, pv[r] - ev[r], ev[r]);
        }
        *(f32x4*)(m + i) = mv;
        *(f32x4*)(v + i) = vv;
        if (AMS) *(f32x4*)(vmax + i) = vm;
        *(f32x4*)(p + i) = pv;
        if (EMA) *(f32x4*)(e + i) = ev;
    } else {
        for (; i < n; ++i, nib >>= 1) {
            float gv = g[i] * gscale;
            float mv = m[i] * b1 + (1.f - b1) * gv;
            float vv = v[i] * b2 + (1.f - b2) * gv * gv;
            float vm = AMS ? fmaxf(vmax[i], vv) : vv;
            m[i] = mv; v[i] = vv;
            if (AMS) vmax[i] = vm;
            float pv = p[i];
            if (WD) pv = nib & 1u ? pv * keep : pv;
            pv -= lr_c1 * (mv / (sqrtf(vm) * inv_sqrt_c2 + eps));
            p[i] = pv;
            if (EMA) e[i] = __builtin_fmaf(w, pv - e[i], e[i]);
        }
    }
}

// any inf / nan among g[0 .. n)?  -> guard[0] = max(guard[0], stamp): one atomic per OFFENDING workgroup, none on a clean gradient
// (an arrival counter on one address cost more than the scan: 2 048 same-address atomics = 30-70 us).  The skipped step is counted
// in guard[1] by the one-thread kernel behind it.  16-byte reads, four in flight per lane.
__global__ __launch_bounds__(256) void grad_nonfinite_kernel(const float* __restrict__ g, int64_t n, unsigned* guard, unsigned stamp) {
    const int64_t stride = (int64_t)gridDim.x * 4096;
    unsigned bad = 0;
    for (int64_t base = (int64_t)blockIdx.x * 4096; base < n; base += stride) {
        const int64_t i0 = base + threadIdx.x * 4;
        if (base + 4096 <= n) {
            u32x4_t b[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) b[u] = *(const u32x4_t*)(g + i0 + u * 1024);
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int r = 0; r < 4; ++r) bad |= ((b[u][r] & 0x7F800000u) == 0x7F800000u);
        } else {
            for (int u = 0; u < 4; ++u)
                for (int64_t j = i0 + u * 1024; j < i0 + u * 1024 + 4 && j < n; ++j)
                    bad |= ((__float_as_uint(g[j]) & 0x7F800000u) == 0x7F800000u);
        }
    }
    const int any = __syncthreads_or((int)bad);
    if (any && threadIdx.x == 0) __hip_atomic_fetch_max(guard, stamp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ void grad_nonfinite_count_kernel(unsigned* guard, unsigned stamp) {      // <<<1, 1>>>, stream-ordered behind the scan
    if (guard[0] == stamp) guard[1] += 1;
}

// Global-norm clipping: part[blockIdx.x] = sum of g[i]^2 over the 4096-element blocks this workgroup walks -- the memory shape of
// grad_nonfinite_kernel (16-byte reads, four in flight per lane, the same grid), and with a guard the same answer about inf / nan
// from the same read.  FIXED ORDER, so the bits depend on (n, values) alone: a lane keeps four running sums, component r of its
// 16-byte reads feeding sum r by one fma per element (4 per trip of the grid-stride loop), then (s0 + s1) + (s2 + s3), wave_sum,
// the four waves through LDS in wave order, one plain store.  No float atomics, no arrival counter.
constexpr int SUMSQ_GRID_CAP = 2048;
static inline int64_t sumsq_grid(int64_t n) { return std::max<int64_t>(1, std::min<int64_t>((n + 4095) / 4096, SUMSQ_GRID_CAP)); }
__global__ __launch_bounds__(256) void grad_sumsq_kernel(const float* __restrict__ g, int64_t n, float* __restrict__ part,
                                                         unsigned* guard, unsigned stamp) {
    __shared__ float red[4];
    const int64_t stride = (int64_t)gridDim.x * 4096;
    unsigned bad = 0;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int64_t base = (int64_t)blockIdx.x * 4096; base < n; base += stride) {
        const int64_t i0 = base + threadIdx.x * 4;
        if (base + 4096 <= n) {
            u32x4_t b[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) b[u] = *(const u32x4_t*)(g + i0 + u * 1024);
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    bad |= ((b[u][r] & 0x7F800000u) == 0x7F800000u);
                    const float x = __uint_as_float(b[u][r]);
                    acc[r] = __builtin_fmaf(x, x, acc[r]);
                }
        } else {
            for (int u = 0; u < 4; ++u)
                for (int r = 0; r < 4; ++r) {
                    const int64_t j = i0 + u * 1024 + r;
                    if (j < n) {
                        const float x = g[j];
                        bad |= ((__float_as_uint(x) & 0x7F800000u) == 0x7F800000u);
                        acc[r] = __builtin_fmaf(x, x, acc[r]);
                    }
                }
        }
    }
    const float s = wave_sum((acc[0] + acc[1]) + (acc[2] + acc[3]));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    const int any = __syncthreads_or((int)bad);
    if (threadIdx.x == 0) {
        part[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
        if (guard && any) __hip_atomic_fetch_max(guard, stamp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// <<<1, 256>>>: the partials of every slice, one behind the other, summed in DOUBLE in a fixed order (thread t takes part[t],
// part[t + 256], ..., then a halving tree through LDS) -> clip[0] = min(1, max_norm / (norm + 1e-6)), clip[1] = norm =
// grad_scale * sqrt(sum): torch.nn.utils.clip_grad_norm_ on the gradient the optimiser consumes.  A NaN norm gives a NaN
// coefficient and an infinite one 0, as torch's clamp does.
__global__ __launch_bounds__(256) void grad_clip_commit_kernel(const float* __restrict__ part, int64_t n_part, float max_norm,
                                                               float gscale, float* __restrict__ clip) {
    __shared__ double red[256];
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < n_part; i += 256) s += (double)part[i];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double norm = (double)gscale * sqrt(red[0]);
        const double c = (double)max_norm / (norm + 1e-6);
        clip[0] = (float)(c > 1.0 ? 1.0 : c);
        clip[1] = (float)norm;
    }
}

// Gradient accumulation over micro-batches (tnr_grad_accum): dst = src (OVERWRITE: dst is never read, so a stale inf / nan in it
// cannot survive, and the pass moves 8 bytes per element) or dst = dst + src (12 bytes per element): one IEEE fp32 add per element,
// no scale, no fma, nothing reassociated - the bits depend on the two inputs alone.  The memory shape of grad_nonfinite_kernel:
// 16-byte accesses, four in flight per lane (eight loads when adding), 4096 elements per workgroup per trip of the grid-stride loop,
// scalars in the last partial block.  dst and src never overlap (the host checks dst != src; slices of two different buffers).
constexpr int ACCUM_GRID_CAP = 2048;
template <bool OVERWRITE>
__global__ __launch_bounds__(256) void grad_accum_kernel(float* __restrict__ dst, const float* __restrict__ src, int64_t n) {
    const int64_t stride = (int64_t)gridDim.x * 4096;
    for (int64_t base = (int64_t)blockIdx.x * 4096; base < n; base += stride) {
        const int64_t i0 = base + threadIdx.x * 4;
        if (base + 4096 <= n) {
            f32x4 s[4], d[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) s[u] = *(const f32x4*)(src + i0 + u * 1024);
            if (!OVERWRITE) {
#pragma unroll
                for (int u = 0; u < 4; ++u) d[u] = *(const f32x4*)(dst + i0 + u * 1024);
#pragma unroll
                for (int u = 0; u < 4; ++u) s[u] = d[u] + s[u];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) *(f32x4*)(dst + i0 + u * 1024) = s[u];
        } else {
            for (int u = 0; u < 4; ++u)
                for (int64_t j = i0 + u * 1024; j < i0 + u * 1024 + 4 && j < n; ++j)
                    dst[j] = OVERWRITE ? src[j] : dst[j] + src[j];
        }
    }
}

}  // namespace

extern "C" int tnr_grad_accum(float* dst, const float* src, int64_t n, int overwrite, void* stream) {
    TNR_CHECK_ARG(dst && src && n >= 1, "tnr_grad_accum: dst and src must not be NULL and n must be at least 1");
    TNR_CHECK_ARG(((uintptr_t)dst % 16) == 0 && ((uintptr_t)src % 16) == 0, "tnr_grad_accum: 16-byte alignment");
    TNR_CHECK_ARG(dst != src, "tnr_grad_accum: dst and src must be different buffers");
    const unsigned grid = (unsigned)std::min<int64_t>((n + 4095) / 4096, ACCUM_GRID_CAP);
    if (overwrite) hipLaunchKernelGGL(grad_accum_kernel<true>, dim3(grid), dim3(256), 0, (hipStream_t)stream, dst, src, n);
    else hipLaunchKernelGGL(grad_accum_kernel<false>, dim3(grid), dim3(256), 0, (hipStream_t)stream, dst, src, n);
    TNR_CHECK_LAUNCH("tnr_grad_accum");
    return TNR_OK;
}

extern "C" int tnr_amsgrad_step(float* p, const float* g, float* m, float* v, float* vmax, int64_t n, int step, float lr,
                                float beta1, float beta2, float eps, float grad_scale, void* stream) {
    return tnr_amsgrad_step_guarded(p, g, m, v, vmax, n, step, lr, beta1, beta2, eps, grad_scale, nullptr, 0u, 0u, stream);
}

extern "C" int tnr_grad_nonfinite_scan(const float* g, int64_t n, unsigned* guard, unsigned stamp, void* stream) {
    TNR_CHECK_ARG(g && guard && n >= 1 && stamp >= 1 && ((uintptr_t)g % 16) == 0, "tnr_grad_nonfinite_scan: bad argument");
    const unsigned grid = (unsigned)std::min<int64_t>((n + 4095) / 4096, 2048);
    hipLaunchKernelGGL(grad_nonfinite_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, g, n, guard, stamp);
    TNR_CHECK_LAUNCH("tnr_grad_nonfinite_scan");
    return TNR_OK;
}

extern "C" int tnr_grad_nonfinite_commit(unsigned* guard, unsigned stamp, void* stream) {
    TNR_CHECK_ARG(guard && stamp >= 1, "tnr_grad_nonfinite_commit: bad argument");
    hipLaunchKernelGGL(grad_nonfinite_count_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, guard, stamp);
    TNR_CHECK_LAUNCH("tnr_grad_nonfinite_commit");
    return TNR_OK;
}

extern "C" int tnr_grad_nonfinite(const float* g, int64_t n, unsigned* guard, unsigned stamp, void* stream) {
    TNR_CHECK_ARG(g && guard && n >= 1 && stamp >= 1 && ((uintptr_t)g % 16) == 0, "tnr_grad_nonfinite: bad argument");
    const unsigned grid = (unsigned)std::min<int64_t>((n + 4095) / 4096, 2048);
    hipLaunchKernelGGL(grad_nonfinite_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, g, n, guard, stamp);
    hipLaunchKernelGGL(grad_nonfinite_count_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, guard, stamp);
    TNR_CHECK_LAUNCH("tnr_grad_nonfinite");
    return TNR_OK;
}

// lr[k]: the learning rate of candidate k (all three equal without a schedule); weight_decay > 0 needs the decay map; ema: the
// average's buffer and its three weights, or NULL for the update without an average.
static int amsgrad_launch(float* p, const float* g, float* m, float* v, float* vmax, int64_t n, int step, const float* lr,
                          float beta1, float beta2, float eps, float grad_scale, const unsigned* guard, unsigned stamp,
                          unsigned known_skips, const float* clip, float weight_decay, const unsigned* decay_bits, int64_t first,
                          const AdamEma* ema, void* stream) {
    TNR_CHECK_ARG(p && g && m && v && n >= 1 && step >= 1, "tnr_amsgrad_step: bad argument");     // vmax NULL = plain Adam
    TNR_CHECK_ARG(((uintptr_t)p % 16) == 0 && ((uintptr_t)g % 16) == 0 && ((uintptr_t)m % 16) == 0 &&
                      ((uintptr_t)v % 16) == 0 && ((uintptr_t)vmax % 16) == 0, "tnr_amsgrad_step: 16-byte alignment");
    const bool wd = weight_decay != 0.f;
    AdamFactors f;
    AdamDecay d;
    for (int k = 0; k < 3; ++k) {
        const int t = step - k >= 1 ? step - k : 1;
        const double c1 = 1.0 - pow((double)beta1, t), c2 = 1.0 - pow((double)beta2, t);
        f.lr_c1[k] = (float)((double)lr[k] / c1);
        f.inv_sqrt_c2[k] = (float)(1.0 / sqrt(c2));
        d.lr_wd[k] = (float)((double)lr[k] * (double)weight_decay);
    }
    f.known_skips = known_skips;
    const AdamEma a = ema ? *ema : AdamEma{nullptr, {0.f, 0.f, 0.f}};
    int64_t nthr = (n + 3) / 4;
    const dim3 grid((unsigned)((nthr + 255) / 256));
#define TNR_AMSGRAD_LAUNCH(AMS, CLIP, WD, EMA)                                                                                   \
    hipLaunchKernelGGL((amsgrad_kernel<AMS, CLIP, WD, EMA>), grid, dim3(256), 0, (hipStream_t)stream, p, g, m, v, vmax, n, f,    \
                       beta1, beta2, eps, grad_scale, guard, stamp, clip, decay_bits, first, d, a)
#define TNR_AMSGRAD_LAUNCH_EMA(AMS, CLIP, WD)                                                                                    \
    do { if (ema) TNR_AMSGRAD_LAUNCH(AMS, CLIP, WD, true); else TNR_AMSGRAD_LAUNCH(AMS, CLIP, WD, false); } while (0)
#define TNR_AMSGRAD_LAUNCH_WD(AMS, CLIP)                                                                                         \
    do { if (wd) TNR_AMSGRAD_LAUNCH_EMA(AMS, CLIP, true); else TNR_AMSGRAD_LAUNCH_EMA(AMS, CLIP, false); } while (0)
    if (vmax) {
        if (clip) TNR_AMSGRAD_LAUNCH_WD(true, true);
        else TNR_AMSGRAD_LAUNCH_WD(true, false);
    } else {  // plain Adam (Post-train_KD.ipynb cell 18: optim.Adam without amsgrad)
        if (clip) TNR_AMSGRAD_LAUNCH_WD(false, true);
        else TNR_AMSGRAD_LAUNCH_WD(false, false);
    }
#undef TNR_AMSGRAD_LAUNCH_WD
#undef TNR_AMSGRAD_LAUNCH_EMA
#undef TNR_AMSGRAD_LAUNCH
    TNR_CHECK_LAUNCH("tnr_amsgrad_step");
    return TNR_OK;
}

extern "C" int tnr_amsgrad_step_guarded(float* p, const float* g, float* m, float* v, float* vmax, int64_t n, int step, float lr,
                                        float beta1, float beta2, float eps, float grad_scale, const unsigned* guard,
                                        unsigned stamp, unsigned known_skips, void* stream) {
    const float lrs[3] = {lr, lr, lr};
    return amsgrad_launch(p, g, m, v, vmax, n, step, lrs, beta1, beta2, eps, grad_scale, guard, stamp, known_skips, nullptr, 0.f,
                          nullptr, 0, nullptr, stream);
}

extern "C" int tnr_amsgrad_step_clipped(float* p, const float* g, float* m, float* v, float* vmax, int64_t n, int step, float lr,
                                        float beta1, float beta2, float eps, float grad_scale, const unsigned* guard,
                                        unsigned stamp, unsigned known_skips, const float* clip, void* stream) {
    TNR_CHECK_ARG(clip && ((uintptr_t)clip % 4) == 0, "tnr_amsgrad_step_clipped: clip must point at the two floats of tnr_grad_clip_commit");
    const float lrs[3] = {lr, lr, lr};
    return amsgrad_launch(p, g, m, v, vmax, n, step, lrs, beta1, beta2, eps, grad_scale, guard, stamp, known_skips, clip, 0.f,
                          nullptr, 0, nullptr, stream);
}

// tnr_adamw_step and tnr_adamw_step_ema (ema != NULL): one set of checks, one launcher
static int adamw_step(float* p, const float* g, float* m, float* v, float* vmax, int64_t n, int step, float lr0, float lr1,
                      float lr2, float beta1, float beta2, float eps, float grad_scale, float weight_decay,
                      const unsigned* decay_bits, int64_t first, const unsigned* guard, unsigned stamp, unsigned known_skips,
                      const float* clip, const AdamEma* ema, void* stream) {
    TNR_CHECK_ARG(weight_decay >= 0.f && (weight_decay == 0.f || decay_bits) && ((uintptr_t)decay_bits % 4) == 0,
                  "tnr_adamw_step: weight_decay > 0 needs the decay map (and none below 0)");
    TNR_CHECK_ARG(first >= 0 && first % 4 == 0, "tnr_adamw_step: first must be a multiple of 4 (a thread's four bits in one word)");
    TNR_CHECK_ARG(((uintptr_t)clip % 4) == 0, "tnr_adamw_step: clip must point at the two floats of tnr_grad_clip_commit");
    const float lrs[3] = {lr0, lr1, lr2};
    return amsgrad_launch(p, g, m, v, vmax, n, step, lrs, beta1, beta2, eps, grad_scale, guard, stamp, known_skips, clip,
                          weight_decay, decay_bits, first, ema, stream);
}

extern "C" int tnr_adamw_step(float* p, const float* g, float* m, float* v, float* vmax, int64_t n, int step, float lr0, float lr1,
                              float lr2, float beta1, float beta2, float eps, float grad_scale, float weight_decay,
                              const unsigned* decay_bits, int64_t first, const unsigned* guard, unsigned stamp,
                              unsigned known_skips, const float* clip, void* stream) {
    return adamw_step(p, g, m, v, vmax, n, step, lr0, lr1, lr2, beta1, beta2, eps, grad_scale, weight_decay, decay_bits, first,
                      guard, stamp, known_skips, clip, nullptr, stream);
}

extern "C" int tnr_adamw_step_ema(float* p, const float* g, float* m, float* v, float* vmax, int64_t n, int step, float lr0,
                                  float lr1, float lr2, float beta1, float beta2, float eps, float grad_scale, float weight_decay,
                                  const unsigned* decay_bits, int64_t first, const unsigned* guard, unsigned stamp,
                                  unsigned known_skips, const float* clip, float* ema, float w0, float w1, float w2, void* stream) {
    TNR_CHECK_ARG(ema && ((uintptr_t)ema % 16) == 0, "tnr_adamw_step_ema: ema must be a 16-byte aligned buffer laid out like p");
    TNR_CHECK_ARG(w0 >= 0.f && w0 <= 1.f && w1 >= 0.f && w1 <= 1.f && w2 >= 0.f && w2 <= 1.f,     // false for a NaN
                  "tnr_adamw_step_ema: every weight 1 - decay must lie in [0, 1]");
    const AdamEma a = {ema, {w0, w1, w2}};
    return adamw_step(p, g, m, v, vmax, n, step, lr0, lr1, lr2, beta1, beta2, eps, grad_scale, weight_decay, decay_bits, first,
                      guard, stamp, known_skips, clip, &a, stream);
}

extern "C" int64_t tnr_grad_sumsq_parts(int64_t n) { return sumsq_grid(n); }

extern "C" int tnr_grad_sumsq_scan(const float* g, int64_t n, float* part, unsigned* guard, unsigned stamp, void* stream) {
    TNR_CHECK_ARG(g && part && n >= 1 && ((uintptr_t)g % 16) == 0 && (!guard || stamp >= 1), "tnr_grad_sumsq_scan: bad argument");
    hipLaunchKernelGGL(grad_sumsq_kernel, dim3((unsigned)sumsq_grid(n)), dim3(256), 0, (hipStream_t)stream, g, n, part, guard, stamp);
    TNR_CHECK_LAUNCH("tnr_grad_sumsq_scan");
    return TNR_OK;
}

extern "C" int tnr_grad_clip_commit(const float* part, int64_t n_part, float max_norm, float grad_scale, float* clip, void* stream) {
    TNR_CHECK_ARG(part && clip && n_part >= 1 && max_norm > 0.f, "tnr_grad_clip_commit: bad argument");
    hipLaunchKernelGGL(grad_clip_commit_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, part, n_part, max_norm, grad_scale, clip);
    TNR_CHECK_LAUNCH("tnr_grad_clip_commit");
    return TNR_OK;
}
