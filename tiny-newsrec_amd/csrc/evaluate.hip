// Rank metrics of the eval path on the device (tnr_rank_metrics): per impression, the scores of its candidate rows against its
// user vector and AUC / MRR / nDCG@5 / nDCG@10 of the labels under those scores; per launch, their totals.  fp32 scores, double
// metrics: built once (ONCE in the Makefile).
//
// rm_impression_kernel: one wave (a 64-thread workgroup) per impression.  The user vector goes to LDS once.  The candidates are
// taken 64 at a time, a lane per candidate; their news rows are gathered through LDS in chunks of 64 k - 16 consecutive lanes read
// the 256 bytes of one row's chunk, two full cache lines - with the next chunk's loads in flight under this chunk's arithmetic.
// A score is the fp32 fma chain over k = 0, 1, 2, ... from +0 (retrieve.hip's definition: the exact fp32 MFMA is that chain, bit
// for bit), run by the candidate's lane alone, so its bits depend on (user row, news row, D) and on nothing else.  The scores go
// to `scores`; the rank phase reads them back from there, so an impression may have any number of candidates.
// Rank phase (rm_rank): only positives need a position.  For each positive i, in index order, the wave counts over all j
//   r_i = #{s_j > s_i} + #{j > i, s_j == s_i}   and   2 #{negatives s_j < s_i} + #{negatives s_j == s_i}
// as integers (a wave sum of integers has no order), and every lane adds the same double terms in the same order.
// rm_total_kernel: one workgroup sums the per-impression values in a fixed order - thread t the impressions t, t + 256, ... in
// turn, then a fixed tree over the threads - so the totals are bit-identical from run to run without a float atomic.  Without a
// `per` buffer there is nowhere to keep an impression's values, and that workgroup computes them again from `scores`, 256
// impressions at a time through LDS, and sums them in the same order (the slow form: callers that care pass `per`).
#include "common.h"
#include <math.h>

namespace {

constexpr int RM_MAX_D = 1024;
constexpr int RM_KC = 64;                  // k values per staged chunk
constexpr int RM_LD = RM_KC + 1;           // padded LDS row: the 64 lanes' reads at one k fall on distinct banks
constexpr int RM_PIECES = RM_KC / 4;       // 16-byte pieces of a row's chunk = lanes per row
constexpr int RM_NLD = 64 * RM_PIECES / 64;    // pieces per lane and chunk: 16
constexpr int RM_TT = 256;                 // threads of the totals workgroup

struct RankArgs {
    const float* users; int64_t u_rs; int64_t B;
    const float* news; int64_t n_rs; int64_t Nn;
    int D;
    const int32_t* offs; const int32_t* cand; const int32_t* label;
    float* scores; double* per;
    int vec;                               // both operands allow 16-byte loads
};

__device__ __forceinline__ unsigned rm_wave_sum(unsigned v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += (unsigned)__shfl_xor((int)v, o, 64);
    return v;
}

// four floats at p, which holds element k of a row of D: one 16-byte load where the launch allows it and the row has all four
__device__ __forceinline__ f32x4 rm_load4(const float* p, int k, int D, bool vec) {
    if (vec && k + 4 <= D) return *(const f32x4*)p;
    f32x4 v;
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = k + e < D ? p[e] : 0.f;
    return v;
}

__device__ __forceinline__ double rm_gain(unsigned r) { return 1.0 / log2((double)(r + 2u)); }

// AUC, MRR, nDCG@5, nDCG@10 of one impression from its scores s[0:C] and labels y[0:C]; the whole wave calls it and every lane
// returns the same values.  false (and zeros) when the impression has no positive or no negative.
__device__ bool rm_rank(const float* __restrict__ s, const int32_t* __restrict__ y, int C, int lane, double out[4]) {
    out[0] = out[1] = out[2] = out[3] = 0.0;
    unsigned p = 0;
    for (int j = lane; j < C; j += 64) p += y[j] != 0;
    const unsigned P = rm_wave_sum(p), Q = (unsigned)C - P;
    if (C <= 0 || P == 0u || Q == 0u) return false;
    unsigned long long a2 = 0ull;          // sum over positives of 2 #{negatives below} + #{negatives equal}
    double mrr = 0.0, d5 = 0.0, d10 = 0.0;
    for (int i0 = 0; i0 < C; i0 += 64) {
        const int i = i0 + lane;
        const bool pos = i < C && y[i] != 0;
        const float si = i < C ? s[i] : 0.f;
        unsigned long long m = __ballot(pos);
        while (m != 0ull) {                                          // wave-uniform: one turn per positive, in index order
            const int src = __ffsll((long long)m) - 1;
            m &= m - 1ull;
            const float sv = __shfl(si, src, 64);
            const int ii = i0 + src;
            unsigned r = 0u, a = 0u;
            for (int j = lane; j < C; j += 64) {
                const float sj = s[j];
                const bool neg = y[j] == 0;
                r += (sj > sv) || (sj == sv && j > ii);
                a += neg ? (sj < sv ? 2u : (sj == sv ? 1u : 0u)) : 0u;
            }
            r = rm_wave_sum(r);
            a2 += rm_wave_sum(a);
            mrr += 1.0 / (double)(r + 1u);
            if (r < 10u) {
                const double g = rm_gain(r);
                d10 += g;
                if (r < 5u) d5 += g;
            }
        }
    }
    double i5 = 0.0, i10 = 0.0;
    for (unsigned t = 0; t < 10u && t < P; ++t) {
        const double g = rm_gain(t);
        i10 += g;
        if (t < 5u) i5 += g;
    }
    out[0] = 0.5 * (double)a2 / ((double)P * (double)Q);
    out[1] = mrr / (double)P;
    out[2] = d5 / i5;
    out[3] = d10 / i10;
    return true;
}

template <bool METRICS>
__global__ __launch_bounds__(64) void rm_impression_kernel(RankArgs g) {
    __shared__ float Us[RM_MAX_D];
    __shared__ float Ns[64 * RM_LD];
    const int lane = threadIdx.x;
    const int64_t b = blockIdx.x;
    const int64_t c0 = g.offs[b];
    const int64_t cw = (int64_t)g.offs[b + 1] - c0;
    const int C = cw > 0 ? (int)cw : 0;
    const int D = g.D;
    const bool vec = g.vec != 0;
    const int kp = (lane & (RM_PIECES - 1)) * 4;                     // this lane's piece of every row chunk
    const int r0 = lane / RM_PIECES;                                 // its rows of a tile: r0, r0 + 4, ...

    const float* up = g.users + b * g.u_rs;
    for (int k = lane * 4; k < D; k += 256) {
        const f32x4 v = rm_load4(up + k, k, D, vec);
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (k + e < D) Us[k + e] = v[e];
    }

    const int nkc = (D + RM_KC - 1) / RM_KC;
    for (int t0 = 0; t0 < C; t0 += 64) {
        const int j = t0 + lane;
        int64_t row = -1;
        if (j < C) {
            row = g.cand[c0 + j];
            if (row < 0 || row >= g.Nn) row = -1;                    // never read: the score is NaN
        }
        int rid[RM_NLD];
#pragma unroll
        for (int q = 0; q < RM_NLD; ++q) rid[q] = __shfl((int)row, r0 + 4 * q, 64);

        f32x4 nv[RM_NLD];
        auto fetch = [&](int kc) {
            const int k = kc * RM_KC + kp;
#pragma unroll
            for (int q = 0; q < RM_NLD; ++q)
                nv[q] = (rid[q] >= 0 && k < D) ? rm_load4(g.news + (int64_t)rid[q] * g.n_rs + k, k, D, vec) : f32x4{0.f, 0.f, 0.f, 0.f};
        };
        float acc = 0.f;
        fetch(0);
        for (int kc = 0; kc < nkc; ++kc) {
#pragma unroll
            for (int q = 0; q < RM_NLD; ++q) {
                float* d = Ns + (r0 + 4 * q) * RM_LD + kp;
                d[0] = nv[q][0]; d[1] = nv[q][1]; d[2] = nv[q][2]; d[3] = nv[q][3];
            }
            __syncthreads();
            if (kc + 1 < nkc) fetch(kc + 1);                         // the next chunk's loads fly under this chunk's chain
            const int k0 = kc * RM_KC;
            const int kn = D - k0 < RM_KC ? D - k0 : RM_KC;
            const float* np = Ns + lane * RM_LD;
            const float* uq = Us + k0;
            if (kn == RM_KC) {
#pragma unroll 16
                for (int kk = 0; kk < RM_KC; ++kk) acc = __builtin_fmaf(np[kk], uq[kk], acc);      // k ascending
            } else {
                for (int kk = 0; kk < kn; ++kk) acc = __builtin_fmaf(np[kk], uq[kk], acc);
            }
            __syncthreads();
        }
        if (j < C) g.scores[c0 + j] = row >= 0 ? acc : __uint_as_float(0x7fc00000u);
    }
    if (METRICS) {
        __syncthreads();                                             // the wave's own scores, back from memory
        double out[4];
        rm_rank(g.scores + c0, g.label + c0, C, lane, out);
        if (lane < 4) g.per[b * 4 + lane] = lane == 0 ? out[0] : lane == 1 ? out[1] : lane == 2 ? out[2] : out[3];
    }
}

// acc[6] (+)= {B, impressions scored, sum AUC, sum MRR, sum nDCG@5, sum nDCG@10}.  FROM_PER: the values are per's (an impression
// was scored iff its MRR is positive: it has a positive, at some finite position); else they are computed here from `scores`.
template <bool FROM_PER>
__global__ __launch_bounds__(RM_TT) void rm_total_kernel(RankArgs g, double* __restrict__ acc, int accumulate) {
    __shared__ double red[5][RM_TT];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    double t[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int64_t base = 0; base < g.B; base += RM_TT) {
        const int64_t b = base + tid;
        double v[4] = {0.0, 0.0, 0.0, 0.0};
        if (FROM_PER) {
            if (b < g.B) {
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = g.per[b * 4 + e];
            }
        } else {
            const int64_t end = base + RM_TT < g.B ? base + RM_TT : g.B;
            for (int64_t x = base + w; x < end; x += RM_TT / 64) {
                const int64_t c0 = g.offs[x];
                const int64_t cw = (int64_t)g.offs[x + 1] - c0;
                double out[4];
                rm_rank(g.scores + c0, g.label + c0, cw > 0 ? (int)cw : 0, lane, out);
                if (lane < 4) red[lane][x - base] = lane == 0 ? out[0] : lane == 1 ? out[1] : lane == 2 ? out[2] : out[3];
            }
            __syncthreads();
            if (b < g.B) {
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = red[e][tid];
            }
            __syncthreads();
        }
        t[0] += v[1] > 0.0 ? 1.0 : 0.0;
#pragma unroll
        for (int e = 0; e < 4; ++e) t[1 + e] += v[e];
    }
#pragma unroll
    for (int e = 0; e < 5; ++e) red[e][tid] = t[e];
    for (int s = RM_TT / 2; s > 0; s >>= 1) {
        __syncthreads();
        if (tid < s) {
#pragma unroll
            for (int e = 0; e < 5; ++e) red[e][tid] += red[e][tid + s];
        }
    }
    __syncthreads();
    if (tid < 6) {
        const double x = tid == 0 ? (double)g.B : red[tid - 1][0];
        acc[tid] = accumulate ? acc[tid] + x : x;
    }
}

}  // namespace

extern "C" int tnr_rank_metrics(const float* users, int64_t u_rs, int64_t B, const float* news, int64_t n_rs, int64_t Nn, int D,
                                const int32_t* offs, const int32_t* cand, const int32_t* label, float* scores, double* per,
                                double* acc, int accumulate, void* stream) {
    TNR_CHECK_ARG(acc, "tnr_rank_metrics: null pointer (acc)");
    TNR_CHECK_ARG(B >= 0 && B < (1ll << 31) && Nn >= 0 && Nn < (1ll << 31), "tnr_rank_metrics: bad sizes (B %ld, Nn %ld)", (long)B, (long)Nn);
    TNR_CHECK_ARG(D >= 1 && D <= RM_MAX_D, "tnr_rank_metrics: D = %d outside 1..%d", D, RM_MAX_D);
    TNR_CHECK_ARG(B == 0 || (users && news && offs && cand && label && scores), "tnr_rank_metrics: null pointer");
    TNR_CHECK_ARG(B == 0 || (u_rs >= D && n_rs >= D), "tnr_rank_metrics: row strides %ld / %ld below D = %d", (long)u_rs, (long)n_rs, D);
    TNR_CHECK_ARG(((uintptr_t)acc & 7) == 0 && ((uintptr_t)per & 7) == 0, "tnr_rank_metrics: acc and per must be 8-byte aligned");
    RankArgs g{users, u_rs, B, news, n_rs, Nn, D, offs, cand, label, scores, per,
               (((uintptr_t)users | (uintptr_t)news) & 15) == 0 && u_rs % 4 == 0 && n_rs % 4 == 0};
    hipStream_t st = (hipStream_t)stream;
    if (B > 0) {
        if (per) hipLaunchKernelGGL(rm_impression_kernel<true>, dim3((unsigned)B), dim3(64), 0, st, g);
        else hipLaunchKernelGGL(rm_impression_kernel<false>, dim3((unsigned)B), dim3(64), 0, st, g);
        TNR_CHECK_LAUNCH("tnr_rank_metrics");
    }
    if (per) hipLaunchKernelGGL(rm_total_kernel<true>, dim3(1), dim3(RM_TT), 0, st, g, acc, accumulate);
    else hipLaunchKernelGGL(rm_total_kernel<false>, dim3(1), dim3(RM_TT), 0, st, g, acc, accumulate);
    TNR_CHECK_LAUNCH("tnr_rank_metrics/total");
    return TNR_OK;
}
