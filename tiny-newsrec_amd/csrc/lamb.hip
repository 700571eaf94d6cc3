// LAMB (You et al., "Large Batch Optimization for Deep Learning", Algorithm 2) over the flat trainable-parameter buffer, fp32:
// per-tensor trust ratios ||w|| / ||u|| on top of the Adam / AMSGrad moments of optim.hip.  Three launches per step:
//   lamb_norm_kernel    per chunk: sum w^2 and sum u^2 of the WOULD-BE update, nothing stored but two partials
//   lamb_commit_kernel  per tensor: the partials in double -> trust, ||w||, ||u||
//   lamb_apply_kernel   per chunk: the same u again (same expressions, same bits), moments stored, w -= lr_k trust u, the average
// The contract (semantics, guard, clip, determinism): include/tnr_hip.h.
//
// The flat buffer has no per-tensor map: slots of a group lie back to back, a tensor starts at any element offset.  The host
// (engine.lamb_chunks) cuts every trainable tensor into chunks (first element, count <= 4096, tensor, flags), none across a
// tensor's end; gaps and reserved rows belong to no chunk and are neither read nor written.  One workgroup per chunk: a scalar
// head up to the first 16-byte boundary of the ABSOLUTE address, 16-byte accesses, a scalar tail.
#include <math.h>

#include "common.h"

// every product-sum below is an explicit fma or an explicit two-step: the norm pass and the apply pass must form u with the same
// bits, so nothing is left for the compiler to contract one way in one kernel and another way in the other
#pragma clang fp contract(off)

namespace {

constexpr int LAMB_CHUNK = 4096;         // elements per chunk at most: 256 lanes x 4 x 16 bytes
constexpr int LAMB_TENSOR_MAX = 1 << 20;

struct LambChunk { int first, count, tensor, flags; };      // flags bit 0: the tensor is in the decay set (adapted, u += wd w)
struct LambTensor { int first_chunk, n_chunks, adapted, pad; };

// candidates k = 0, 1, 2 (t_k = max(step - k, 1) updates taken, this one included), picked by guard[1] - known_skips as
// amsgrad_kernel picks: inv_c1 = 1 / (1 - b1^t), inv_sqrt_c2 = 1 / sqrt(1 - b2^t), formed on the host in double
struct LambFactors { float inv_c1[3], inv_sqrt_c2[3]; unsigned known_skips; };
struct LambRates { float lr[3]; };
struct LambEma { float* e; float w[3]; };

struct LambConst { float b1, omb1, b2, omb2, eps, gscale, inv_c1, inv_sqrt_c2, wd; };

// guard / candidate pick shared by the norm and the apply pass: false = this launch is the skipped step
__device__ __forceinline__ bool lamb_pick(const unsigned* __restrict__ guard, unsigned stamp, unsigned known_skips, int& k) {
    k = 0;
    if (guard) {
        if (guard[0] == stamp) return false;
        const unsigned d = guard[1] - known_skips;
        k = d == 0 ? 0 : (d == 1 ? 1 : 2);
    }
    return true;
}

// one element: new moments and the update direction u (r = (m / c1) / (sqrt(vhat) / sqrt(c2) + eps), + wd w in the decay set)
template <bool AMS>
__device__ __forceinline__ float lamb_elem(float w, float g, float m, float v, float vmax, const LambConst& c, bool decay,
                                           float& m2, float& v2, float& vm2) {
    const float gs = g * c.gscale;
    m2 = __builtin_fmaf(m, c.b1, c.omb1 * gs);
    v2 = __builtin_fmaf(v, c.b2, (c.omb2 * gs) * gs);
    vm2 = AMS ? fmaxf(vmax, v2) : v2;
    const float den = __builtin_fmaf(sqrtf(vm2), c.inv_sqrt_c2, c.eps);
    const float r = c.inv_c1 * (m2 / den);
    return decay ? __builtin_fmaf(c.wd, w, r) : r;
}

// the walk of a chunk, shared by both passes: body(i) for a 16-byte group at element i, one(i) for a single element
// head: [first, a0), vectors: [a0, a1) by fours, tail: [a1, end)
struct LambSpan { int64_t first, a0, a1, end; };
__device__ __forceinline__ LambSpan lamb_span(const LambChunk c) {
    LambSpan s;
    s.first = c.first;
    s.end = (int64_t)c.first + c.count;
    const int64_t up = ((int64_t)c.first + 3) & ~(int64_t)3;
    s.a0 = up < s.end ? up : s.end;
    s.a1 = s.a0 + ((s.end - s.a0) & ~(int64_t)3);
    return s;
}

template <bool AMS>
__global__ __launch_bounds__(256) void lamb_norm_kernel(const float* __restrict__ p, const float* __restrict__ g,
                                                        const float* __restrict__ m, const float* __restrict__ v,
                                                        const float* __restrict__ vmax, const LambChunk* __restrict__ chunks,
                                                        LambFactors f, float b1, float b2, float eps, float gscale, float wd,
                                                        const unsigned* __restrict__ guard, unsigned stamp,
                                                        const float* __restrict__ clip, float* __restrict__ part) {
    __shared__ float red[2][4];
    int k;
    if (!lamb_pick(guard, stamp, f.known_skips, k)) return;
    const LambChunk ch = chunks[blockIdx.x];
    if (!(ch.flags & 1)) return;                        // not adapted: trust = 1, no norm wanted
    if (clip) gscale *= clip[0];
    const LambConst c = {b1, 1.f - b1, b2, 1.f - b2, eps, gscale, f.inv_c1[k], f.inv_sqrt_c2[k], wd};
    const bool decay = wd != 0.f;
    const LambSpan s = lamb_span(ch);
    f32x4 aw = {0.f, 0.f, 0.f, 0.f}, au = {0.f, 0.f, 0.f, 0.f};
    float m2, v2, vm2;
    const int t = threadIdx.x;
    // scalars first: lane t takes head element t (< 3 of them) and tail element t (< 4 of them), into component 0
    if (s.first + t < s.a0) {
        const int64_t i = s.first + t;
        const float w = p[i];
        const float u = lamb_elem<AMS>(w, g[i], m[i], v[i], AMS ? vmax[i] : 0.f, c, decay, m2, v2, vm2);
        aw[0] = __builtin_fmaf(w, w, aw[0]);
        au[0] = __builtin_fmaf(u, u, au[0]);
    }
    if (s.a1 + t < s.end) {
        const int64_t i = s.a1 + t;
        const float w = p[i];
        const float u = lamb_elem<AMS>(w, g[i], m[i], v[i], AMS ? vmax[i] : 0.f, c, decay, m2, v2, vm2);
        aw[0] = __builtin_fmaf(w, w, aw[0]);
        au[0] = __builtin_fmaf(u, u, au[0]);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {                        // at most 1024 vectors: four per lane
        const int64_t i = s.a0 + ((int64_t)q * 256 + t) * 4;
        if (i < s.a1) {
            const f32x4 pv = *(const f32x4*)(p + i), gv = *(const f32x4*)(g + i), mv = *(const f32x4*)(m + i),
                        vv = *(const f32x4*)(v + i);
            f32x4 xv = vv;
            if (AMS) xv = *(const f32x4*)(vmax + i);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float u = lamb_elem<AMS>(pv[r], gv[r], mv[r], vv[r], xv[r], c, decay, m2, v2, vm2);
                aw[r] = __builtin_fmaf(pv[r], pv[r], aw[r]);
                au[r] = __builtin_fmaf(u, u, au[r]);
            }
        }
    }
    const float sw = wave_sum((aw[0] + aw[1]) + (aw[2] + aw[3]));
    const float su = wave_sum((au[0] + au[1]) + (au[2] + au[3]));
    if ((t & 63) == 0) { red[0][t >> 6] = sw; red[1][t >> 6] = su; }
    __syncthreads();
    if (t == 0) {
        part[2 * (int64_t)blockIdx.x] = ((red[0][0] + red[0][1]) + red[0][2]) + red[0][3];
        part[2 * (int64_t)blockIdx.x + 1] = ((red[1][0] + red[1][1]) + red[1][2]) + red[1][3];
    }
}

// <<<n_tensors, 64>>>: lane l sums the tensor's partials l, l + 64, ... in double, then a butterfly in double - a fixed order.
// out: trust[t], then ||w|| at out[n_tensors + t], then ||u|| at out[2 n_tensors + t]
__global__ __launch_bounds__(64) void lamb_commit_kernel(const float* __restrict__ part, const LambTensor* __restrict__ tensors,
                                                         int n_tensors, float* __restrict__ out,
                                                         const unsigned* __restrict__ guard, unsigned stamp) {
    if (guard && guard[0] == stamp) return;
    const LambTensor tn = tensors[blockIdx.x];
    double sw = 0.0, su = 0.0;
    if (tn.adapted)
        for (int j = threadIdx.x; j < tn.n_chunks; j += 64) {
            sw += (double)part[2 * ((int64_t)tn.first_chunk + j)];
            su += (double)part[2 * ((int64_t)tn.first_chunk + j) + 1];
        }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        sw += __shfl_xor(sw, o, 64);
        su += __shfl_xor(su, o, 64);
    }
    if (threadIdx.x == 0) {
        const double wn = sqrt(sw), un = sqrt(su);
        // both norms > 0: the ratio; a zero norm: 1 (a zero tensor may leave zero, a zero update divides nothing); NaN / inf propagate
        const double tr = (!tn.adapted || wn == 0.0 || un == 0.0) ? 1.0 : wn / un;
        out[blockIdx.x] = (float)tr;
        out[(int64_t)n_tensors + blockIdx.x] = (float)wn;
        out[2 * (int64_t)n_tensors + blockIdx.x] = (float)un;
    }
}

template <bool AMS, bool EMA>
__global__ __launch_bounds__(256) void lamb_apply_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                         float* __restrict__ v, float* __restrict__ vmax,
                                                         const LambChunk* __restrict__ chunks, LambFactors f, LambRates lr,
                                                         float b1, float b2, float eps, float gscale, float wd,
                                                         const unsigned* __restrict__ guard, unsigned stamp,
                                                         const float* __restrict__ clip, const float* __restrict__ trust,
                                                         LambEma a) {
    int k;
    if (!lamb_pick(guard, stamp, f.known_skips, k)) return;
    const LambChunk ch = chunks[blockIdx.x];
    if (clip) gscale *= clip[0];
    const LambConst c = {b1, 1.f - b1, b2, 1.f - b2, eps, gscale, f.inv_c1[k], f.inv_sqrt_c2[k], wd};
    const bool decay = (ch.flags & 1) && wd != 0.f;
    const float nlt = -(lr.lr[k] * trust[ch.tensor]);   // w <- w - lr_k trust u: one fma per element
    const float ew = EMA ? a.w[k] : 0.f;
    float* __restrict__ e = EMA ? a.e : nullptr;
    const LambSpan s = lamb_span(ch);
    const int t = threadIdx.x;
#pragma unroll
    for (int side = 0; side < 2; ++side) {
        const int64_t i = (side ? s.a1 : s.first) + t;
        if (i < (side ? s.end : s.a0)) {
            float m2, v2, vm2;
            const float w = p[i];
            const float u = lamb_elem<AMS>(w, g[i], m[i], v[i], AMS ? vmax[i] : 0.f, c, decay, m2, v2, vm2);
            const float w2 = __builtin_fmaf(nlt, u, w);
            m[i] = m2; v[i] = v2;
            if (AMS) vmax[i] = vm2;
            p[i] = w2;
            if (EMA) e[i] = __builtin_fmaf(ew, w2 - e[i], e[i]);
        }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int64_t i = s.a0 + ((int64_t)q * 256 + t) * 4;
        if (i < s.a1) {
            f32x4 pv = *(const f32x4*)(p + i), mv = *(const f32x4*)(m + i), vv = *(const f32x4*)(v + i);
            const f32x4 gv = *(const f32x4*)(g + i);
            f32x4 xv = vv, ev = pv;
            if (AMS) xv = *(const f32x4*)(vmax + i);
            if (EMA) ev = *(const f32x4*)(e + i);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float m2, v2, vm2;
                const float u = lamb_elem<AMS>(pv[r], gv[r], mv[r], vv[r], xv[r], c, decay, m2, v2, vm2);
                pv[r] = __builtin_fmaf(nlt, u, pv[r]);
                mv[r] = m2; vv[r] = v2; xv[r] = vm2;
                if (EMA) ev[r] = __builtin_fmaf(ew, pv[r] - ev[r], ev[r]);
            }
            *(f32x4*)(m + i) = mv;
            *(f32x4*)(v + i) = vv;
            if (AMS) *(f32x4*)(vmax + i) = xv;
            *(f32x4*)(p + i) = pv;
            if (EMA) *(f32x4*)(e + i) = ev;
        }
    }
}

LambFactors lamb_factors(int step, float beta1, float beta2, unsigned known_skips) {
    LambFactors f;
    for (int k = 0; k < 3; ++k) {
        const int t = step - k >= 1 ? step - k : 1;
        f.inv_c1[k] = (float)(1.0 / (1.0 - pow((double)beta1, t)));
        f.inv_sqrt_c2[k] = (float)(1.0 / sqrt(1.0 - pow((double)beta2, t)));
    }
    f.known_skips = known_skips;
    return f;
}

// the host's copy of the chunks a launch walks: every one inside [0, n), 1 .. 4096 elements, a tensor below n_tensors
bool lamb_chunks_ok(const int32_t* h, int64_t n_chunks, int64_t n, int n_tensors) {
    for (int64_t j = 0; j < n_chunks; ++j) {
        const int64_t first = h[4 * j], count = h[4 * j + 1], tensor = h[4 * j + 2];
        if (first < 0 || count < 1 || count > LAMB_CHUNK || first + count > n || tensor < 0 || tensor >= n_tensors) return false;
    }
    return true;
}

}  // namespace

#define TNR_LAMB_CHECK_COMMON(who)                                                                                              \
    TNR_CHECK_ARG(p && g && m && v && n >= 1 && n < ((int64_t)1 << 31) && step >= 1, who ": bad argument");                      \
    TNR_CHECK_ARG(((uintptr_t)p % 16) == 0 && ((uintptr_t)g % 16) == 0 && ((uintptr_t)m % 16) == 0 &&                            \
                      ((uintptr_t)v % 16) == 0 && ((uintptr_t)vmax % 16) == 0, who ": 16-byte alignment");                       \
    TNR_CHECK_ARG(chunks && chunks_host && ((uintptr_t)chunks % 16) == 0 && n_chunks >= 1 && n_chunks < ((int64_t)1 << 31) &&    \
                      n_tensors >= 1 && n_tensors <= LAMB_TENSOR_MAX,                                                            \
                  who ": the chunk table (device and host copy) and at least one chunk and one tensor");                         \
    TNR_CHECK_ARG(weight_decay >= 0.f, who ": weight_decay must not be negative");                                               \
    TNR_CHECK_ARG(((uintptr_t)clip % 4) == 0 && (!guard || stamp >= 1), who ": clip / guard");                                   \
    TNR_CHECK_ARG(lamb_chunks_ok(chunks_host, n_chunks, n, n_tensors),                                                           \
                  who ": a chunk lies outside [0, n), holds no or more than 4096 elements, or names a tensor >= n_tensors")

extern "C" int tnr_lamb_norms(const float* p, const float* g, const float* m, const float* v, const float* vmax, int64_t n,
                              const int32_t* chunks, const int32_t* chunks_host, int64_t n_chunks, int n_tensors, int step,
                              float beta1, float beta2, float eps, float grad_scale, float weight_decay, const unsigned* guard,
                              unsigned stamp, unsigned known_skips, const float* clip, float* part, void* stream) {
    TNR_LAMB_CHECK_COMMON("tnr_lamb_norms");
    TNR_CHECK_ARG(part && ((uintptr_t)part % 4) == 0, "tnr_lamb_norms: part must hold 2 floats per chunk");
    const LambFactors f = lamb_factors(step, beta1, beta2, known_skips);
    const dim3 grid((unsigned)n_chunks);
    if (vmax)
        hipLaunchKernelGGL(lamb_norm_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, p, g, m, v, vmax,
                           (const LambChunk*)chunks, f, beta1, beta2, eps, grad_scale, weight_decay, guard, stamp, clip, part);
    else
        hipLaunchKernelGGL(lamb_norm_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, p, g, m, v, vmax,
                           (const LambChunk*)chunks, f, beta1, beta2, eps, grad_scale, weight_decay, guard, stamp, clip, part);
    TNR_CHECK_LAUNCH("tnr_lamb_norms");
    return TNR_OK;
}

extern "C" int tnr_lamb_commit(const float* part, int64_t n_chunks, const int32_t* tensors, const int32_t* tensors_host,
                               int n_tensors, float* trust, const unsigned* guard, unsigned stamp, void* stream) {
    TNR_CHECK_ARG(part && tensors && tensors_host && trust && n_chunks >= 1 && n_tensors >= 1 && n_tensors <= LAMB_TENSOR_MAX &&
                      ((uintptr_t)tensors % 16) == 0 && (!guard || stamp >= 1), "tnr_lamb_commit: bad argument");
    for (int t = 0; t < n_tensors; ++t) {
        const int64_t fc = tensors_host[4 * t], nc = tensors_host[4 * t + 1];
        TNR_CHECK_ARG(fc >= 0 && nc >= 1 && fc + nc <= n_chunks, "tnr_lamb_commit: tensor %d's chunks lie outside [0, n_chunks)", t);
    }
    hipLaunchKernelGGL(lamb_commit_kernel, dim3((unsigned)n_tensors), dim3(64), 0, (hipStream_t)stream, part,
                       (const LambTensor*)tensors, n_tensors, trust, guard, stamp);
    TNR_CHECK_LAUNCH("tnr_lamb_commit");
    return TNR_OK;
}

extern "C" int tnr_lamb_step(float* p, const float* g, float* m, float* v, float* vmax, int64_t n, const int32_t* chunks,
                             const int32_t* chunks_host, int64_t n_chunks, int n_tensors, int step, float lr0, float lr1, float lr2,
                             float beta1, float beta2, float eps, float grad_scale, float weight_decay, const unsigned* guard,
                             unsigned stamp, unsigned known_skips, const float* clip, const float* trust, float* ema, float w0,
                             float w1, float w2, void* stream) {
    TNR_LAMB_CHECK_COMMON("tnr_lamb_step");
    TNR_CHECK_ARG(trust && ((uintptr_t)trust % 4) == 0, "tnr_lamb_step: trust must be the table tnr_lamb_commit wrote");
    TNR_CHECK_ARG(((uintptr_t)ema % 16) == 0, "tnr_lamb_step: ema must be a 16-byte aligned buffer laid out like p");
    if (ema)
        TNR_CHECK_ARG(w0 >= 0.f && w0 <= 1.f && w1 >= 0.f && w1 <= 1.f && w2 >= 0.f && w2 <= 1.f,     // false for a NaN
                      "tnr_lamb_step: every weight 1 - decay must lie in [0, 1]");
    const LambFactors f = lamb_factors(step, beta1, beta2, known_skips);
    const LambRates lr = {{lr0, lr1, lr2}};
    const LambEma a = {ema, {w0, w1, w2}};
    const dim3 grid((unsigned)n_chunks);
#define TNR_LAMB_APPLY(AMS, EMA)                                                                                                 \
    hipLaunchKernelGGL((lamb_apply_kernel<AMS, EMA>), grid, dim3(256), 0, (hipStream_t)stream, p, g, m, v, vmax,                 \
                       (const LambChunk*)chunks, f, lr, beta1, beta2, eps, grad_scale, weight_decay, guard, stamp, clip, trust, a)
    if (vmax) { if (ema) TNR_LAMB_APPLY(true, true); else TNR_LAMB_APPLY(true, false); }
    else { if (ema) TNR_LAMB_APPLY(false, true); else TNR_LAMB_APPLY(false, false); }
#undef TNR_LAMB_APPLY
    TNR_CHECK_LAUNCH("tnr_lamb_step");
    return TNR_OK;
}
