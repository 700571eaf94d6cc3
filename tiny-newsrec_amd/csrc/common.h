// Shared device/host helpers for libtnr_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <atomic>
#include <stdint.h>
#include <stdio.h>

#include "../../include/tnr_hip.h"

// The 16-bit activation type.  The typed sources (TYPED in the Makefile) are compiled twice: once with bf16 (entry points
// tnr_*) and once with -DTNR_BUILD_F16 (IEEE half, entry points tnr_*_f16, same MFMA rate, 3 more mantissa bits).  The
// identifier `bf16` below means "the 16-bit type of this build".  Everything else (ONCE in the Makefile) is fp32 or host code
// and is built once; this header is the only place that tests the switch.
#ifdef TNR_BUILD_F16
typedef _Float16 bf16;
#define TNR_NAME(x) x##_f16
#define TNR_MFMA_16x16x32 __builtin_amdgcn_mfma_f32_16x16x32_f16
#define TNR_MFMA_32x32x16 __builtin_amdgcn_mfma_f32_32x32x16_f16
#else
typedef __bf16 bf16;
#define TNR_NAME(x) x
#define TNR_MFMA_16x16x32 __builtin_amdgcn_mfma_f32_16x16x32_bf16
#define TNR_MFMA_32x32x16 __builtin_amdgcn_mfma_f32_32x32x16_bf16
#endif
typedef __attribute__((ext_vector_type(8))) bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) bf16 bf16x4;
typedef __attribute__((ext_vector_type(2))) bf16 bf16x2;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) short s16x4;

#define WAVE 64

void tnr_set_error(const char* fmt, ...);

// Process-wide GEMM options (api.cpp).  Defaults are the product configuration; only tools/ change them, through
// tnr_gemm_set_option(), for same-process A/B runs.  The library never reads environment variables.
struct TnrGemmOpts {
    int ver;         // 3 = route by shape (default) ; 1 / 2 = force the 128x128 / 256x128 kernels
    int gm;          // rasterisation group height in row tiles
    int fine_pct;    // 256x256 grid fill (percent of the CUs) below which the 128x128 kernel is used
    int allow_fine;  // 0 = never fall back to the 128x128 kernel for sparse grids
    int bm;          // 0 = pick the tile height per launch ; 224 / 256 = force it
    int pp;          // NT: non-zero (default 1) = the persistent ping-pong kernel on the 256x256 routes, 0 = never the queue-fed
                     // kernel (those launches take the 256x128 / 128x128 kernels, which need no tile-queue slot)
    int tnpp;        // weight gradient: non-zero (default 2) = the persistent register-staged kernel, 0 = never the queue-fed kernel
                     // (the 256x128 kernel instead)
    int mix;         // ping-pong NT kernel: 1 = row panels of two heights so that the tiles fill whole rounds, 0 = one height
    int cus;         // 0 = plan and size the persistent GEMM grids for the device's CUs ; n = for n of them (two kernels side by side)
    void* clock_buf; // tnr_gemm_clock_stamps: device buffer of clock_n (cycles, 100 MHz ticks) pairs the persistent NT kernel fills, or NULL
    int clock_n;
};
TnrGemmOpts* tnr_gemm_opts();

// Runs `body` once per device of this process (function attributes such as the dynamic LDS limit are set per device); two
// threads racing through it both run the idempotent body.
#define TNR_ONCE_PER_DEVICE(body)                                                       \
    do {                                                                                \
        static std::atomic<unsigned long long> tnr_done_{0};                            \
        int tnr_dev_ = 0;                                                               \
        (void)hipGetDevice(&tnr_dev_);                                                  \
        const unsigned long long tnr_bit_ = 1ull << (tnr_dev_ & 63);                    \
        if (!(tnr_done_.load(std::memory_order_acquire) & tnr_bit_)) {                  \
            body;                                                                       \
            tnr_done_.fetch_or(tnr_bit_, std::memory_order_release);                    \
        }                                                                               \
    } while (0)

#define TNR_CHECK_ARG(cond, ...)          \
    do {                                  \
        if (!(cond)) {                    \
            tnr_set_error(__VA_ARGS__);   \
            return TNR_EINVAL;            \
        }                                 \
    } while (0)

// public dropout descriptor (host memory, may be NULL = off) -> kernel argument
#include "dropout.h"
static inline int tnr_make_drop(const tnr_dropout_t* d, TnrDrop* o, const char* who) {
    *o = TnrDrop{0u, 0u, 0u, 0u, 0u, 1.0f, 0u, 0xFFFFFFFFu};
    if (!d || d->p <= 0.0) return TNR_OK;
    if (!(d->p < 1.0)) { tnr_set_error("%s: dropout p must be in [0, 1)", who); return TNR_EINVAL; }
    o->k0 = (uint32_t)d->seed;
    o->k1 = (uint32_t)(d->seed >> 32);
    o->site = d->site;
    o->call = d->call;
    o->thresh = (uint32_t)(d->p * 65536.0 + 0.5);
    // p below 2^-17 rounds to "keep everything": then nothing is scaled either (forward kernels test thresh, backward ones
    // multiply by scale -- both must see the same effective dropout)
    o->scale = o->thresh ? (float)(1.0 / (1.0 - d->p)) : 1.0f;
    return TNR_OK;
}
// a row-major site split at row `split` of M: rows [0, split) under `d`, rows [split, M) under `tail` (same seed / site / p,
// its own call; rows counted from split) - the masks of the two passes' own launches.  tail NULL or split == M: `d` alone.
static inline int tnr_make_drop_split(const tnr_dropout_t* d, const tnr_dropout_t* tail, int64_t split, int64_t M, TnrDrop* o,
                                      const char* who) {
    if (int rc = tnr_make_drop(d, o, who)) return rc;
    if (split < 0 || split > M || M > (int64_t)0xFFFFFFFF) { tnr_set_error("%s: split row %ld outside [0, %ld]", who, (long)split, (long)M); return TNR_EINVAL; }
    if (!tail || split == M) return TNR_OK;
    if (!d || d->seed != tail->seed || d->site != tail->site || d->p != tail->p) {
        tnr_set_error("%s: the two halves of a split site must share seed, site and p", who);
        return TNR_EINVAL;
    }
    o->call_tail = tail->call;
    o->split = (uint32_t)split;
    return TNR_OK;
}

#define TNR_CHECK_LAUNCH(name)                                                   \
    do {                                                                         \
        hipError_t e_ = hipGetLastError();                                       \
        if (e_ != hipSuccess) {                                                  \
            tnr_set_error("%s: launch failed: %s", name, hipGetErrorString(e_)); \
            return TNR_ELAUNCH;                                                  \
        }                                                                        \
    } while (0)

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// erf by Abramowitz-Stegun 7.1.26 (|abs err| <= 1.5e-7, far below the bf16 rounding of the outputs):
// one v_rcp + one v_exp + 6 FMAs instead of libm erff's branches.  e = exp(-z*z) is returned for reuse.
// tanh for the additive-attention pre-activations (model_bert.py:25, :37): 1 - 2 / (e^2x + 1) on the hardware exp2 / rcp, an odd
// polynomial below |x| = 0.06 where that form cancels.  |error| <= 3e-7 (libm's tanhf: ~1e-7, at ~60 instructions with divergent
// branches - it made the tanh epilogue of the pooling GEMM cost as much as its K loop and was a third of the user-encoder
// kernel).  ONE function for every kernel: a news vector must not depend on which tile kernel encoded it.
__device__ __forceinline__ float tnr_tanh(float x) {
    const float x2 = x * x;
    const float p = x * (1.f - x2 * (0.33333334f - x2 * 0.13333334f));
    const float t = 1.f - 2.f * __frcp_rn(__expf(2.f * x) + 1.f);
    return fabsf(x) < 0.06f ? p : t;
}

__device__ __forceinline__ float erf_as(float z, float& e) {
    float a = fabsf(z);
    float t = __frcp_rn(1.0f + 0.3275911f * a);
    e = __expf(-a * a);
    float p = t * (0.254829592f + t * (-0.284496736f + t * (1.421413741f + t * (-1.453152027f + t * 1.061405429f))));
    float r = 1.0f - p * e;
    return z < 0.f ? -r : r;
}
// erf-GELU of transformers' BertIntermediate (call site tnlrv3/modeling.py:305) and its derivative
__device__ __forceinline__ float gelu_erf(float x) {
    float e;
    return 0.5f * x * (1.0f + erf_as(x * 0.70710678118654752f, e));
}
__device__ __forceinline__ float gelu_erf_grad(float x) {
    float e;                                  // e = exp(-x*x/2): also the Gaussian pdf's exponential
    float cdf = 0.5f * (1.0f + erf_as(x * 0.70710678118654752f, e));
    return cdf + x * e * 0.39894228040143268f;
}

// async global -> LDS, 16 bytes per lane; LDS destination = wave-uniform base + lane*16
__device__ __forceinline__ void glds16(const void* gsrc, void* lds_wave_base) {
    __builtin_amdgcn_global_load_lds((const void __attribute__((address_space(1)))*)gsrc,
                                     (void __attribute__((address_space(3)))*)lds_wave_base, 16, 0, 0);
}

// transposed LDS read: per 16-lane group a 4-row x 16-col block of 16-bit elements, delivered
// column-major (lane i gets column i, rows 0..3); lane 4q+p supplies the address of row q, cols 4p..4p+3.
__device__ __forceinline__ bf16x4 ds_read_tr16(const void* lds_ptr) {
    return __builtin_bit_cast(bf16x4, __builtin_amdgcn_ds_read_tr16_b64_v4i16((s16x4 __attribute__((address_space(3)))*)lds_ptr));
}

// ---- shared between the typed sources (built twice) and the once-built ones ---------------------------------------------
// A typed launcher that needs an fp32 kernel calls the once-built side through one of the `*_launch` helpers below: they launch
// and nothing else, the caller checks (TNR_CHECK_LAUNCH) under its own name.

// LayerNorm backward (norm_embed.hip; workspace sizes: util_f32.hip)
constexpr int LNB_ROWS = 128;  // rows per block (8 half waves x 16 rows); short inputs use 32 so that every CU gets work
static inline int lnb_rows(int64_t M) { return M >= 32768 ? LNB_ROWS : 32; }
static inline int64_t lnb_blocks(int64_t M) { return (M + lnb_rows(M) - 1) / lnb_rows(M); }

// embedding-LayerNorm backward (norm_embed.hip; workspace sizes: util_f32.hip): tokens per block (four waves, a token per wave
// and turn); short inputs use 16 so that every CU gets work
static inline int embwd_rows(int64_t n_tok) { return n_tok >= 32768 ? 64 : 16; }
static inline int64_t embwd_blocks(int64_t n_tok) { return (n_tok + embwd_rows(n_tok) - 1) / embwd_rows(n_tok); }

// column sums: block = 256 columns (64 threads x 4) x 4 row lanes over `rows_per_block` rows: 512 for tall inputs, 64 for short
// ones (a 1792-row input on 512-row blocks was 4 workgroups walking 128 dependent loads each: 33 us for 1.8 MB)
constexpr int CS_ROWS = 512;
static inline int cs_rows(int64_t M) { return M >= 32768 ? CS_ROWS : 64; }
namespace {
template <typename T>
__global__ __launch_bounds__(256) void colsum_kernel(const T* __restrict__ Xb, int64_t ldx, int64_t M, int64_t N,
                                                     float* __restrict__ partb, int64_t sX, int64_t sPart, int rows_per_block) {
    const T* X = Xb + (int64_t)blockIdx.z * sX;
    float* part = partb + (int64_t)blockIdx.z * sPart;
    // thread handles 4 consecutive columns; 64 threads across 256 columns, 4 row groups
    __shared__ float red[4][256];
    const int cg = threadIdx.x & 63, rg = threadIdx.x >> 6;
    const int64_t c = (int64_t)blockIdx.x * 256 + cg * 4;
    const int64_t m0 = (int64_t)blockIdx.y * rows_per_block;
    float s[4] = {0.f, 0.f, 0.f, 0.f};
    if (c < N) {
        int64_t mend = m0 + rows_per_block < M ? m0 + rows_per_block : M;
        for (int64_t m = m0 + rg; m < mend; m += 4) {
            if constexpr (sizeof(T) == 2) {
                bf16x4 a = *(const bf16x4*)((const bf16*)X + m * ldx + c);
#pragma unroll
                for (int r = 0; r < 4; ++r) s[r] += (float)a[r];
            } else {
                f32x4 a = *(const f32x4*)((const float*)X + m * ldx + c);
#pragma unroll
                for (int r = 0; r < 4; ++r) s[r] += a[r];
            }
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) red[rg][cg * 4 + r] = s[r];
    __syncthreads();
    int t = threadIdx.x;
    int64_t col = (int64_t)blockIdx.x * 256 + t;
    if (col < N) part[(int64_t)blockIdx.y * gridDim.z * N + col] = red[0][t] + red[1][t] + red[2][t] + red[3][t];
}
}  // namespace
void colsum_f32_launch(dim3 grid, const float* X, int64_t ldx, int64_t M, int64_t N, float* part, int64_t sX, int rows_per_block,
                       hipStream_t st);                                   // colsum_kernel<float>: util_f32.hip

// attention pooling of few, long sequences (attpool.hip): tokens per chunk, and the stages without 16-bit data (heads.hip)
constexpr int AP_CH = 64;
void attpool_long_score_launch(const float* e, int64_t lde, const float* w2, const float* b2, int Q, float* alpha, int64_t n_tok,
                               int L, hipStream_t st);
void attpool_long_fwd_fin_launch(const float* ws, float* alpha, float* nv, float* den, int64_t n_seq, int L, int H, hipStream_t st);
void attpool_long_bwd_fin_launch(const float* part, int Q, int64_t lddpre, int nch, float* dw2_part, float* db2_part,
                                 float* db1_part, int64_t n_seq, hipStream_t st);

// GEMM host state and planning (gemm_plan.hip), one copy for both builds of gemm.hip.
// A tile-queue counter set: 8 tile counters + the count of workgroups that have left, each on a 256-byte line of its own.
constexpr int PP_Q_STRIDE = 64;
constexpr int PP_Q_SET = 9 * PP_Q_STRIDE;
constexpr int PP_QUEUE_SETS = 128;
// The counter set of (current device, stream); reset = zero it again (stream-ordered).  NULL + tnr_last_error when the table is full.
unsigned* tnr_pp_queue_of(void* stream, bool reset);
int device_cus();                                                          // option `cus`, or the current device's
struct PpPlan { int mi, P, x; };                                           // instance (32 mi rows), row panels, tall ones among them
PpPlan pp_plan(int64_t M, int64_t N, int flags, int n_cu);
int nt_route(int64_t M, int64_t N, int64_t K, int flags, int n_cu);        // TNR_ROUTE_*
constexpr int TN_MAXP = 4;                                                 // weight gradients per grouped launch
// unit ranges of the eight XCD labels, xb[9], from ubase[TN_MAXP + 1] (first unit of each problem, then the total) and tiles_per_split[n]
void tn_group_ranges(const int* ubase, const int* tiles_per_split, int n, int* xb);
// one slab sum: out[N, K] (ld ldo) (+)= out_scale * sum of `splits` slabs of NK = N * K floats at ws (NK == 0: nothing to do)
struct SlabSum { const float* ws; float* out; int64_t NK, ldo; int splits, K, accumulate; float out_scale; };
void slab_reduce_launch(const SlabSum& s, hipStream_t st);
void slab_reduce_group_launch(const SlabSum* s, int n, hipStream_t st);    // n <= TN_MAXP sums in one launch
