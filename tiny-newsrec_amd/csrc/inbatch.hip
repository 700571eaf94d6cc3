// In-batch negatives of the target loss (tnr_inbatch_plan / tnr_inbatch_loss / tnr_inbatch_bwd; include/tnr_hip.h has the
// definition).  fp32 and integers only: built once (ONCE in the Makefile).  No float atomics: every sum has one owner and one order.
//
// ib_first_kernel / ib_elig_kernel (tnr_inbatch_plan): a thread per slot.  The first writes rule 3's bit of every slot - a nonzero
// news id that no earlier slot holds - as the ballot words of its waves; the second, one workgroup per impression, ands in rules
// 1, 4 and 5 (another impression's slot, an id among neither its own candidates nor its history) and counts the bits it set.
// ib_loss_kernel: one workgroup per impression.  The user vector and the impression's eligibility words go to LDS once.  The
// slots are taken 256 at a time, a lane per slot; the rows of the ELIGIBLE slots are gathered through LDS in chunks of 32 k - 8
// consecutive lanes read the 128 bytes of one row's chunk - with the next chunk's loads in flight under this chunk's arithmetic
// (evaluate.hip's rm_impression_kernel); a row that is eligible for nobody is never read.  A logit is the fp32 fma chain over
// k = 0, 1, 2, ... from +0, run by the slot's lane alone: retrieve.hip's and evaluate.hip's bits for the same pair.  The raw
// logits wait in the impression's own dz row (each lane reads back only what it wrote).  Sum of exponentials: thread t its own
// candidate t (t < C) and then the eligible slots of RANK t, t + 256, ... among the impression's eligible slots, then a fixed
// tree over the threads - by rank and not by slot number, so that an impression's loss has the same bits wherever its negatives
// sit in the batch (the max has no order).
// ib_mean_kernel: one workgroup sums the per-impression losses in a fixed order (rm_total_kernel's) into losses[1].
// ib_bwd_kernel: workgroups [0, B) own the user rows, [B, B + B*C) the candidate rows; threads over D, set bits in ascending order.
#include "common.h"

namespace {

constexpr int IB_MAX_D = 1024;
constexpr int IB_MAX_SLOTS = 8192;
constexpr int IB_MAX_C = 16;
constexpr int IB_T = 256;                      // threads of every workgroup here = slots per round
constexpr int IB_KC = 32;                      // k values per staged chunk
constexpr int IB_LD = IB_KC + 1;               // padded LDS row: a wave's reads at one k fall on distinct banks
constexpr int IB_PIECES = IB_KC / 4;           // 16-byte pieces of a row's chunk = lanes per row
constexpr int IB_ROWS = IB_T / IB_PIECES;      // rows one pass of the workgroup loads: 32
constexpr int IB_NLD = IB_T / IB_ROWS;         // passes (pieces per thread) per chunk: 8
constexpr float IB_NEG = -3.0e38f;

// the two 32-bit words of a wave's ballot go to words 2 * wave, 2 * wave + 1 of a row of W words (slot0 = the wave's first slot)
__device__ __forceinline__ void ib_store_ballot(unsigned long long m, uint32_t* __restrict__ row, int64_t slot0, int64_t W, int lane) {
    const int64_t w = slot0 / 32 + (lane >> 5);
    if ((lane & 31) == 0 && w < W) row[w] = (uint32_t)(m >> (lane & 32));
}

__global__ __launch_bounds__(IB_T) void ib_first_kernel(const int32_t* __restrict__ cand, uint32_t* __restrict__ first, int64_t M,
                                                        int64_t W) {
    const int64_t j = (int64_t)blockIdx.x * IB_T + threadIdx.x;
    bool f = false;
    if (j < M) {
        const int32_t n = cand[j];
        f = n != 0;
        for (int64_t i = 0; f && i < j; ++i) f = cand[i] != n;
    }
    const unsigned long long m = __ballot(f);
    ib_store_ballot(m, first, j - (threadIdx.x & 63), W, threadIdx.x & 63);
}

__global__ __launch_bounds__(IB_T) void ib_elig_kernel(const int32_t* __restrict__ hist, const int32_t* __restrict__ cand,
                                                       const uint32_t* __restrict__ first, uint32_t* __restrict__ elig,
                                                       int32_t* __restrict__ count, int U, int C, int64_t M, int64_t W) {
    __shared__ int red[IB_T];
    const int64_t b = blockIdx.x;
    const int32_t* own = cand + b * C;
    const int32_t* hb = hist + b * U;
    const int lane = threadIdx.x & 63;
    int n_set = 0;
    for (int64_t base = 0; base < W * 32; base += IB_T) {
        const int64_t j = base + threadIdx.x;
        bool e = false;
        if (j < M && j / C != b && ((first[j >> 5] >> (j & 31)) & 1u)) {
            const int32_t n = cand[j];
            e = true;
            for (int c = 0; e && c < C; ++c) e = own[c] != n;
            for (int u = 0; e && u < U; ++u) e = hb[u] != n;
        }
        n_set += e;
        ib_store_ballot(__ballot(e), elig + b * W, j - lane, W, lane);
    }
    red[threadIdx.x] = n_set;
    for (int s = IB_T / 2; s > 0; s >>= 1) {
        __syncthreads();
        if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    }
    if (threadIdx.x == 0) count[b] = red[0];
}

struct IbLoss {
    const float* users; int64_t u_rs;
    const float* cands; int64_t c_rs;
    const float* score; const int64_t* label; const uint32_t* elig;
    float coef;
    float* dscore; float* dz; float* z; float* per;
    int B, C, D, M, W;
    int vec;                                   // both operands allow 16-byte loads
};

// four floats at p (element k of a row of D, D % 4 == 0 and k % 4 == 0, so all four exist)
__device__ __forceinline__ f32x4 ib_load4(const float* p, bool vec) {
    if (vec) return *(const f32x4*)p;
    return f32x4{p[0], p[1], p[2], p[3]};
}

// max / sum over the workgroup in a fixed order; every thread returns the result
template <bool MAX>
__device__ __forceinline__ float ib_block_reduce(float v, float* red) {
    __syncthreads();                           // red may still be read from the reduction before
    red[threadIdx.x] = v;
    for (int s = IB_T / 2; s > 0; s >>= 1) {
        __syncthreads();
        if (threadIdx.x < s) red[threadIdx.x] = MAX ? fmaxf(red[threadIdx.x], red[threadIdx.x + s]) : red[threadIdx.x] + red[threadIdx.x + s];
    }
    __syncthreads();
    return red[0];
}

__global__ __launch_bounds__(IB_T) void ib_loss_kernel(IbLoss g) {
    __shared__ float Us[IB_MAX_D];
    __shared__ float Ns[IB_T * IB_LD];
    __shared__ uint32_t Es[IB_MAX_SLOTS / 32];
    __shared__ int Ps[IB_MAX_SLOTS / 32];
    __shared__ int wtot[IB_T / 64];
    __shared__ float red[IB_T];
    static_assert(IB_MAX_SLOTS / 32 == IB_T && IB_T * IB_LD >= IB_MAX_SLOTS, "a word per thread; Ns holds every slot's exponential");
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x;
    const int D = g.D, M = g.M, C = g.C;
    const bool vec = g.vec != 0;
    const int kp = (tid & (IB_PIECES - 1)) * 4;                       // this thread's piece of every row chunk
    const int r0 = tid / IB_PIECES;                                   // its rows of a round: r0, r0 + 32, ...

    const float* up = g.users + b * g.u_rs;
    for (int k = tid * 4; k < D; k += IB_T * 4) {
        const f32x4 v = ib_load4(up + k, vec);
        Us[k] = v[0]; Us[k + 1] = v[1]; Us[k + 2] = v[2]; Us[k + 3] = v[3];
    }
    // W <= 256 words, one per thread: Ps[w] = the bits set in the words before w (an exclusive scan of integers), n_elig their total
    const uint32_t ew = tid < g.W ? g.elig[b * g.W + tid] : 0u;
    Es[tid] = ew;
    int inc = __popc(ew);
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int v = __shfl_up(inc, o, 64);
        if ((tid & 63) >= o) inc += v;
    }
    if ((tid & 63) == 63) wtot[tid >> 6] = inc;
    __syncthreads();
    int before = 0;
    for (int w = 0; w < (tid >> 6); ++w) before += wtot[w];
    Ps[tid] = before + inc - __popc(ew);
    const int n_elig = wtot[0] + wtot[1] + wtot[2] + wtot[3];
    __syncthreads();
    auto bit = [&](int j) { return j < M && ((Es[j >> 5] >> (j & 31)) & 1u) != 0u; };

    float* zrow = g.dz + b * (int64_t)M;                              // raw logits first, their gradients at the end
    const float own = tid < C ? g.score[b * C + tid] : IB_NEG;
    float mx = own;
    const int nkc = (D + IB_KC - 1) / IB_KC;
    for (int base = 0; base < M; base += IB_T) {
        const int j = base + tid;
        const bool e = bit(j);
        bool ld[IB_NLD];
#pragma unroll
        for (int q = 0; q < IB_NLD; ++q) ld[q] = bit(base + r0 + IB_ROWS * q);
        f32x4 nv[IB_NLD];
        auto fetch = [&](int kc) {
            const int k = kc * IB_KC + kp;
#pragma unroll
            for (int q = 0; q < IB_NLD; ++q)
                nv[q] = (ld[q] && k < D) ? ib_load4(g.cands + (int64_t)(base + r0 + IB_ROWS * q) * g.c_rs + k, vec) : f32x4{0.f, 0.f, 0.f, 0.f};
        };
        float acc = 0.f;
        fetch(0);
        for (int kc = 0; kc < nkc; ++kc) {
#pragma unroll
            for (int q = 0; q < IB_NLD; ++q) {
                float* d = Ns + (r0 + IB_ROWS * q) * IB_LD + kp;
                d[0] = nv[q][0]; d[1] = nv[q][1]; d[2] = nv[q][2]; d[3] = nv[q][3];
            }
            __syncthreads();
            if (kc + 1 < nkc) fetch(kc + 1);                          // the next chunk's loads fly under this chunk's chain
            const int k0 = kc * IB_KC;
            const int kn = D - k0 < IB_KC ? D - k0 : IB_KC;
            const float* np = Ns + tid * IB_LD;
            const float* uq = Us + k0;
            if (kn == IB_KC) {
#pragma unroll
                for (int kk = 0; kk < IB_KC; ++kk) acc = __builtin_fmaf(np[kk], uq[kk], acc);      // k ascending
            } else {
                for (int kk = 0; kk < kn; ++kk) acc = __builtin_fmaf(np[kk], uq[kk], acc);
            }
            __syncthreads();
        }
        if (e) {
            zrow[j] = acc;
            if (g.z) g.z[b * (int64_t)M + j] = acc;
            mx = fmaxf(mx, acc);
        }
    }
    mx = ib_block_reduce<true>(mx, red);
    // the exponentials line up in Ns by RANK among the impression's eligible slots (Ns is free: the last chunk's barrier is
    // behind every thread), so the order of the sum does not move when the same negatives sit at other slots of another batch
    for (int j = tid; j < M; j += IB_T)
        if (bit(j)) Ns[Ps[j >> 5] + __popc(Es[j >> 5] & ((1u << (j & 31)) - 1u))] = __expf(zrow[j] - mx);
    __syncthreads();
    // log of the sum as log1p(sum - 1): the terms that are exactly 1 (the largest logit's, and whatever rounds to it) are counted,
    // the others summed, so that a positive that dominates - a loss of 1e-6 - keeps its digits (log(1 + 1e-6) in fp32 keeps one)
    float se = 0.f, ones = 0.f;
    auto take = [&](float v) { if (v == 1.f) ones += 1.f; else se += v; };
    if (tid < C) take(__expf(own - mx));
    for (int r = tid; r < n_elig; r += IB_T) take(Ns[r]);
    se = ib_block_reduce<false>(se, red);
    ones = ib_block_reduce<false>(ones, red);                         // small integers: exact in any order
    const float lse = log1pf((ones - 1.f) + se);
    const float fB = (float)g.B;
    for (int j = tid; j < M; j += IB_T) zrow[j] = bit(j) ? g.coef * __expf(zrow[j] - mx - lse) / fB : 0.f;
    const int64_t y = g.label[b];
    // p - 1 of the positive as expm1: it cancels to nothing exactly where the positive dominates
    if (tid < C) g.dscore[b * C + tid] += g.coef * (tid == y ? expm1f(own - mx - lse) : __expf(own - mx - lse)) / fB;
    if (tid < C && tid == y) g.per[b] = (mx - own) + lse;             // (a label in [C, 256) has a thread, but no candidate)
    if (tid == 0 && (y < 0 || y >= C)) g.per[b] = __uint_as_float(0x7fc00000u);      // no such candidate: NaN, as a bad row scores
}

__global__ __launch_bounds__(IB_T) void ib_mean_kernel(const float* __restrict__ per, float* __restrict__ out, int B) {
    __shared__ float red[IB_T];
    float t = 0.f;
    for (int b = threadIdx.x; b < B; b += IB_T) t += per[b];
    const float s = ib_block_reduce<false>(t, red);
    if (threadIdx.x == 0) *out = s / (float)B;
}

__global__ __launch_bounds__(IB_T) void ib_bwd_kernel(const float* __restrict__ dz, const uint32_t* __restrict__ elig,
                                                      const float* __restrict__ users, int64_t u_rs,
                                                      const float* __restrict__ cands, int64_t c_rs, float* __restrict__ duser,
                                                      float* __restrict__ dcand, int B, int D, int M, int W) {
    if ((int)blockIdx.x < B) {
        const int64_t b = blockIdx.x;
        const uint32_t* eb = elig + b * W;
        const float* zb = dz + b * (int64_t)M;
        for (int d = threadIdx.x; d < D; d += IB_T) {
            float acc = 0.f;
            bool any = false;
            for (int w = 0; w < W; ++w) {
                uint32_t m = eb[w];
                while (m) {                                            // j ascending
                    const int j = w * 32 + __ffs((int)m) - 1;
                    m &= m - 1u;
                    if (j < M) {
                        acc = __builtin_fmaf(zb[j], cands[(int64_t)j * c_rs + d], acc);
                        any = true;
                    }
                }
            }
            if (any) duser[b * D + d] += acc;
        }
    } else {
        const int64_t j = (int64_t)blockIdx.x - B;
        const int w = (int)(j >> 5);
        const uint32_t m = 1u << (j & 31);
        for (int d = threadIdx.x; d < D; d += IB_T) {
            float acc = 0.f;
            bool any = false;
            for (int64_t b = 0; b < B; ++b)                            // b ascending
                if (elig[b * W + w] & m) {
                    acc = __builtin_fmaf(dz[b * M + j], users[b * u_rs + d], acc);
                    any = true;
                }
            if (any) dcand[j * D + d] += acc;
        }
    }
}

}  // namespace

extern "C" int tnr_inbatch_plan(const int32_t* hist_ids, const int32_t* cand_ids, uint32_t* elig, int32_t* count,
                                uint32_t* first_ws, int B, int U, int C, void* stream) {
    TNR_CHECK_ARG(cand_ids && elig && count && first_ws && (U == 0 || hist_ids), "tnr_inbatch_plan: null pointer");
    TNR_CHECK_ARG(B >= 1 && U >= 0 && C >= 1 && (int64_t)B * C <= (1 << 24), "tnr_inbatch_plan: bad shape (B %d, U %d, C %d; B*C <= 2^24)", B, U, C);
    const int64_t M = (int64_t)B * C, W = (M + 31) / 32;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(ib_first_kernel, dim3((unsigned)((W * 32 + IB_T - 1) / IB_T)), dim3(IB_T), 0, st, cand_ids, first_ws, M, W);
    TNR_CHECK_LAUNCH("tnr_inbatch_plan/first");
    hipLaunchKernelGGL(ib_elig_kernel, dim3((unsigned)B), dim3(IB_T), 0, st, hist_ids, cand_ids, first_ws, elig, count, U, C, M, W);
    TNR_CHECK_LAUNCH("tnr_inbatch_plan");
    return TNR_OK;
}

extern "C" int tnr_inbatch_loss(const float* users, int64_t u_rs, const float* cands, int64_t c_rs, const float* score,
                                const int64_t* label, const uint32_t* elig, float coef, float* dscore, float* dz, float* z,
                                float* per, float* losses, int B, int C, int D, void* stream) {
    TNR_CHECK_ARG(users && cands && score && label && elig && dscore && dz && per && losses, "tnr_inbatch_loss: null pointer");
    TNR_CHECK_ARG(B >= 1 && C >= 1 && D >= 4, "tnr_inbatch_loss: bad shape (B %d, C %d, D %d)", B, C, D);
    TNR_CHECK_ARG(C <= IB_MAX_C, "tnr_inbatch_loss: C = %d above %d", C, IB_MAX_C);
    TNR_CHECK_ARG((int64_t)B * C <= IB_MAX_SLOTS, "tnr_inbatch_loss: B*C = %ld above %d slots", (long)B * C, IB_MAX_SLOTS);
    TNR_CHECK_ARG(D <= IB_MAX_D, "tnr_inbatch_loss: D = %d above %d", D, IB_MAX_D);
    TNR_CHECK_ARG(D % 4 == 0, "tnr_inbatch_loss: D = %d is not a multiple of 4", D);
    TNR_CHECK_ARG(u_rs >= D && c_rs >= D, "tnr_inbatch_loss: row strides %ld / %ld below D = %d", (long)u_rs, (long)c_rs, D);
    const int M = B * C;
    IbLoss g{users, u_rs, cands, c_rs, score, label, elig, coef, dscore, dz, z, per, B, C, D, M, (M + 31) / 32,
             (((uintptr_t)users | (uintptr_t)cands) & 15) == 0 && u_rs % 4 == 0 && c_rs % 4 == 0};
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(ib_loss_kernel, dim3((unsigned)B), dim3(IB_T), 0, st, g);
    TNR_CHECK_LAUNCH("tnr_inbatch_loss");
    hipLaunchKernelGGL(ib_mean_kernel, dim3(1), dim3(IB_T), 0, st, per, losses + 1, B);
    TNR_CHECK_LAUNCH("tnr_inbatch_loss/mean");
    return TNR_OK;
}

extern "C" int tnr_inbatch_bwd(const float* dz, const uint32_t* elig, const float* users, int64_t u_rs, const float* cands,
                               int64_t c_rs, float* duser, float* dcand, int B, int C, int D, void* stream) {
    TNR_CHECK_ARG(dz && elig && users && cands && duser && dcand, "tnr_inbatch_bwd: null pointer");
    TNR_CHECK_ARG(B >= 1 && C >= 1 && D >= 1 && (int64_t)B * C <= IB_MAX_SLOTS, "tnr_inbatch_bwd: bad shape (B %d, C %d, D %d; B*C <= %d)",
                  B, C, D, IB_MAX_SLOTS);
    TNR_CHECK_ARG(u_rs >= D && c_rs >= D, "tnr_inbatch_bwd: row strides %ld / %ld below D = %d", (long)u_rs, (long)c_rs, D);
    const int M = B * C;
    hipLaunchKernelGGL(ib_bwd_kernel, dim3((unsigned)(B + M)), dim3(IB_T), 0, (hipStream_t)stream, dz, elig, users, u_rs, cands, c_rs,
                       duser, dcand, B, D, M, (M + 31) / 32);
    TNR_CHECK_LAUNCH("tnr_inbatch_bwd");
    return TNR_OK;
}
