// fp32-only companions of the row kernels (norm_embed.hip) and small utilities: fixed-order row reductions, the fp32 column
// sum, the rel-pos bias table, the dropout-mask accessors of the tests, workspace sizes.  Built once; the typed sources call
// tnr_reduce_rows and colsum_f32_launch.
#include "common.h"

namespace {

// fixed-order sum over rows of a (rows, stride) fp32 matrix.  Wide outputs: block = 64 columns x 4 row lanes
// (each lane a strided subsequence, combined in a fixed order).  Narrow outputs (n < 64): one block per column.
__global__ __launch_bounds__(256) void reduce_rows_kernel(const float* __restrict__ part, int64_t rows, int64_t stride,
                                                          int64_t n, float* __restrict__ out, int accumulate) {
    __shared__ float red[4][64];
    const int c = threadIdx.x & 63, rl = threadIdx.x >> 6;
    const int64_t i = (int64_t)blockIdx.x * 64 + c;
    float s = 0.f;
    if (i < n)
        for (int64_t r = rl; r < rows; r += 4) s += part[r * stride + i];
    red[rl][c] = s;
    __syncthreads();
    if (rl == 0 && i < n) {
        float t = (red[0][c] + red[1][c]) + (red[2][c] + red[3][c]);
        out[i] = accumulate ? out[i] + t : t;
    }
}
// many reductions in one launch: one descriptor per BLOCK on the device, 6 int64
// {src ptr, rows, row stride (floats), ncols <= 64, dst ptr, accumulate | scale bits << 32}: dst[c] (+)= scale * sum_r src[r*stride + c]
// (scale = the fp32 whose bit pattern sits in the upper half of the last word; upper half 0 means 1.0).
// Fixed order (4 row lanes, each a strided subsequence, combined as ((0+1)+(2+3))).  The host builds two tables
// per batch: level 1 sums row chunks IN PLACE (dst = first row of the chunk), level 2 sums the chunk rows.
__global__ __launch_bounds__(256) void reduce_multi_kernel(const int64_t* __restrict__ desc) {
    __shared__ float red[4][64];
    const int64_t* d = desc + (int64_t)blockIdx.x * 6;
    const float* src = (const float*)d[0];
    const int64_t rows = d[1], stride = d[2];
    const int ncols = (int)d[3];
    float* dst = (float*)d[4];
    const int c = threadIdx.x & 63, rl = threadIdx.x >> 6;
    float s0 = 0.f, s1 = 0.f;
    if (c < ncols) {
        int64_t r = rl;
        for (; r + 4 < rows; r += 8) {               // two independent chains: more loads in flight
            s0 += src[r * stride + c];
            s1 += src[(r + 4) * stride + c];
        }
        if (r < rows) s0 += src[r * stride + c];
    }
    red[rl][c] = s0 + s1;
    __syncthreads();
    if (rl == 0 && c < ncols) {
        float t = (red[0][c] + red[1][c]) + (red[2][c] + red[3][c]);
        const unsigned sb = (unsigned)((uint64_t)d[5] >> 32);
        if (sb) t *= __uint_as_float(sb);
        dst[c] = (d[5] & 1) ? dst[c] + t : t;
    }
}

// first level for tall inputs: chunk y sums its rows IN PLACE into its first row (each block only touches its own
// 64 columns of its own chunk), so that the second level reads `chunks` rows instead of `rows`
__global__ __launch_bounds__(256) void reduce_rows_chunk_kernel(float* __restrict__ part, int64_t rows, int64_t stride,
                                                                int64_t n, int64_t chunk) {
    __shared__ float red[4][64];
    const int c = threadIdx.x & 63, rl = threadIdx.x >> 6;
    const int64_t i = (int64_t)blockIdx.x * 64 + c;
    const int64_t r0 = (int64_t)blockIdx.y * chunk;
    const int64_t r1 = r0 + chunk < rows ? r0 + chunk : rows;
    float s = 0.f;
    if (i < n)
        for (int64_t r = r0 + rl; r < r1; r += 4) s += part[r * stride + i];
    red[rl][c] = s;
    __syncthreads();
    if (rl == 0 && i < n) part[r0 * stride + i] = (red[0][c] + red[1][c]) + (red[2][c] + red[3][c]);
}
__global__ __launch_bounds__(256) void reduce_rows_narrow_kernel(const float* __restrict__ part, int64_t rows,
                                                                 int64_t stride, float* __restrict__ out, int accumulate) {
    __shared__ float red[256];
    const int64_t i = blockIdx.x;
    float s = 0.f;
    for (int64_t r = threadIdx.x; r < rows; r += 256) s += part[r * stride + i];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int k = 128; k > 0; k >>= 1) {
        if ((int)threadIdx.x < k) red[threadIdx.x] += red[threadIdx.x + k];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[i] = accumulate ? out[i] + red[0] : red[0];
}

// tnlrv3/modeling.py:345-373 bucket (integer edges, see oracle) + the Linear(32->A) lookup of :462-463
__device__ __forceinline__ int relpos_bucket(int rel) {
    int n = rel < 0 ? -rel : rel;
    int b;
    if (n < 8) b = n;
    else if (n < 12) b = 8;
    else if (n < 16) b = 9;
    else if (n < 23) b = 10;
    else if (n < 32) b = 11;
    else if (n < 46) b = 12;
    else if (n < 64) b = 13;
    else if (n < 91) b = 14;
    else b = 15;
    return (rel > 0 ? 16 : 0) + b;
}
__global__ void relpos_kernel(const float* __restrict__ weight, int A, int L, int Lr, float* __restrict__ table) {
    int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (int64_t)A * Lr * Lr) return;
    int a = (int)(idx / ((int64_t)Lr * Lr));
    int rem = (int)(idx - (int64_t)a * Lr * Lr);
    int i = rem / Lr, j = rem - i * Lr;
    table[idx] = (i < L && j < L) ? weight[a * 32 + relpos_bucket(j - i)] : 0.f;
}

}  // namespace

extern "C" int tnr_relpos_table(const float* weight, int A, int L, float* table, void* stream) {
    TNR_CHECK_ARG(weight && table && A >= 1 && L >= 1 && L <= 512, "tnr_relpos_table: need 1<=L<=512");
    const int Lr = (L + 31) / 32 * 32;        // table is (A, Lr, Lr): (A,32,32) for the fused short kernel
    hipLaunchKernelGGL(relpos_kernel, dim3((unsigned)(((int64_t)A * Lr * Lr + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       weight, A, L, Lr, table);
    TNR_CHECK_LAUNCH("tnr_relpos_table");
    return TNR_OK;
}

// workspace for any row count up to M (short inputs use smaller blocks, i.e. more partial rows)
extern "C" int64_t tnr_ln_bwd_part_elems(int64_t M, int H) {
    int64_t nb = lnb_blocks(M), nb_short = lnb_blocks(M < 32767 ? M : 32767);
    return (nb > nb_short ? nb : nb_short) * 3 * H;
}
extern "C" int64_t tnr_ln_bwd_blocks(int64_t M) { return lnb_blocks(M); }
// the same for tnr_embed_ln_bwd: one [dgamma | dbeta] row of 2 H floats per block
extern "C" int64_t tnr_embed_ln_bwd_part_elems(int64_t n_tok, int H) {
    int64_t nb = embwd_blocks(n_tok), nb_short = embwd_blocks(n_tok < 32767 ? n_tok : 32767);
    return (nb > nb_short ? nb : nb_short) * 2 * H;
}
extern "C" int64_t tnr_embed_ln_bwd_blocks(int64_t n_tok) { return embwd_blocks(n_tok); }

extern "C" int tnr_reduce_rows(const float* part, int64_t rows, int64_t stride, int64_t n, float* out, int accumulate,
                               void* stream) {
    TNR_CHECK_ARG(part && out && rows >= 1 && n >= 1, "tnr_reduce_rows: bad argument");
    // (tests/rows_ref.py::reduce_rows_depth restates this branching for its error bounds: retune the two together)
    const int64_t colblk = (n + 63) / 64;
    if (n < 64 && rows >= 256) {
        hipLaunchKernelGGL(reduce_rows_narrow_kernel, dim3((unsigned)n), dim3(256), 0, (hipStream_t)stream, part, rows,
                           stride, out, accumulate);
    } else if (rows >= 128 && colblk < 512) {
        // two levels: enough workgroups to stream the partials at HBM rate; `part` is clobbered (it is scratch)
        int64_t chunks = 1024 / colblk;
        if (chunks > rows / 16) chunks = rows / 16;
        if (chunks < 2) chunks = 2;
        int64_t chunk = (rows + chunks - 1) / chunks;
        chunks = (rows + chunk - 1) / chunk;
        hipLaunchKernelGGL(reduce_rows_chunk_kernel, dim3((unsigned)colblk, (unsigned)chunks), dim3(256), 0,
                           (hipStream_t)stream, (float*)part, rows, stride, n, chunk);
        hipLaunchKernelGGL(reduce_rows_kernel, dim3((unsigned)colblk), dim3(256), 0, (hipStream_t)stream, part, chunks,
                           chunk * stride, n, out, accumulate);
    } else {
        hipLaunchKernelGGL(reduce_rows_kernel, dim3((unsigned)colblk), dim3(256), 0, (hipStream_t)stream, part, rows,
                           stride, n, out, accumulate);
    }
    TNR_CHECK_LAUNCH("tnr_reduce_rows");
    return TNR_OK;
}

// the fp32 instance of the column sum (common.h) for tnr_colsum_batched of either build; launch only, the caller checks
void colsum_f32_launch(dim3 grid, const float* X, int64_t ldx, int64_t M, int64_t N, float* part, int64_t sX, int rows_per_block,
                       hipStream_t st) {
    hipLaunchKernelGGL(colsum_kernel<float>, grid, dim3(256), 0, st, X, ldx, M, N, part, sX, N, rows_per_block);
}

// monotone in M: a workspace sized for M rows serves every call with fewer rows
extern "C" int64_t tnr_colsum_part_elems(int64_t M, int64_t N) {
    int64_t tall = (M + CS_ROWS - 1) / CS_ROWS, small = (M + 63) / 64;
    if (small > 32768 / 64) small = 32768 / 64;
    return (tall > small ? tall : small) * N;
}

// the multipliers of a dropout site as fp32 (tests: statistics, bit equality with oracle/dropout_oracle.py)
__global__ void dropout_mask_rows_kernel(float* __restrict__ out, int64_t n4, int64_t cols, TnrDrop d) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n4) return;
    float m[4];
    const int64_t row = i * 4 / cols;
    uint32_t dc;
    const uint32_t mr = tnr_drop_row(d, (uint32_t)row, dc);
    tnr_drop4(d, dc, (uint64_t)mr * cols + (i * 4 - row * cols), m);
    *(f32x4*)(out + i * 4) = (f32x4){m[0], m[1], m[2], m[3]};
}
// attention probabilities (pairs, L, L): thread = (pair, query, key group of 4) through the row accessor, or (cols != 0) the
// column accessor (four queries of one key), so both device paths are pinned
__global__ void dropout_mask_probs_kernel(float* __restrict__ out, int64_t pairs, int L, int Lr, int cols, TnrDrop d) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int g = Lr / 4;
    if (i >= pairs * Lr * g) return;
    const int64_t pair = i / ((int64_t)Lr * g);
    const int rem = (int)(i - pair * Lr * g);
    float m[4];
    if (!cols) {
        const int q = rem / g, k0 = (rem - q * g) * 4;
        tnr_drop_prob_row(d, (uint64_t)pair, g, q, k0, m);
        for (int e = 0; e < 4; ++e)
            if (q < L && k0 + e < L) out[(pair * L + q) * L + k0 + e] = m[e];
    } else {
        const int k = rem / g, q0 = (rem - k * g) * 4;
        tnr_drop_prob_col(d, (uint64_t)pair, g, q0, k, m);
        for (int e = 0; e < 4; ++e)
            if (k < L && q0 + e < L) out[(pair * L + q0 + e) * L + k] = m[e];
    }
}
extern "C" int tnr_dropout_mask(const tnr_dropout_t* drop, int64_t rows, int64_t cols, float* out, void* stream) {
    return tnr_dropout_mask_split(drop, nullptr, rows, rows, cols, out, stream);
}
extern "C" int tnr_dropout_mask_split(const tnr_dropout_t* drop, const tnr_dropout_t* drop_tail, int64_t split_row, int64_t rows,
                                      int64_t cols, float* out, void* stream) {
    TnrDrop dd;
    if (int rc = tnr_make_drop_split(drop, drop_tail, split_row, rows, &dd, "tnr_dropout_mask")) return rc;
    TNR_CHECK_ARG(out && rows >= 1 && cols >= 4 && (cols % 4) == 0, "tnr_dropout_mask: need cols %% 4 == 0");
    int64_t n4 = rows * cols / 4;
    hipLaunchKernelGGL(dropout_mask_rows_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, out, n4, cols,
                       dd);
    TNR_CHECK_LAUNCH("tnr_dropout_mask");
    return TNR_OK;
}
extern "C" int tnr_dropout_mask_probs(const tnr_dropout_t* drop, int64_t pairs, int L, int by_columns, float* out, void* stream) {
    TnrDrop dd;
    if (int rc = tnr_make_drop(drop, &dd, "tnr_dropout_mask_probs")) return rc;
    TNR_CHECK_ARG(out && pairs >= 1 && L >= 1 && L <= 512, "tnr_dropout_mask_probs: bad argument");
    const int Lr = (L + 31) / 32 * 32;
    int64_t n = pairs * Lr * (Lr / 4);
    hipLaunchKernelGGL(dropout_mask_probs_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, out, pairs, L,
                       Lr, by_columns, dd);
    TNR_CHECK_LAUNCH("tnr_dropout_mask_probs");
    return TNR_OK;
}
__global__ void scale_inplace_kernel(float* __restrict__ x, int64_t n, float s) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) x[i] *= s;
}
extern "C" int tnr_scale_inplace(float* x, int64_t n, float s, void* stream) {
    TNR_CHECK_ARG(x && n >= 1, "tnr_scale_inplace: bad argument");
    hipLaunchKernelGGL(scale_inplace_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, n, s);
    TNR_CHECK_LAUNCH("tnr_scale_inplace");
    return TNR_OK;
}
extern "C" int tnr_reduce_multi(const int64_t* desc, int n_blocks, void* stream) {
    TNR_CHECK_ARG(desc && n_blocks >= 1, "tnr_reduce_multi: bad argument");
    hipLaunchKernelGGL(reduce_multi_kernel, dim3((unsigned)n_blocks), dim3(256), 0, (hipStream_t)stream, desc);
    TNR_CHECK_LAUNCH("tnr_reduce_multi");
    return TNR_OK;
}
