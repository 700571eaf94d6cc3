// HBM-bound row kernels on the 16-bit activations: embedding gather + LayerNorm, LayerNorm fwd/bwd, pooling, column sums, casts,
// the 16-bit weight copies.  (Their fp32-only companions - row reductions, rel-pos table, workspace sizes - are in util_f32.hip.)
// LayerNorm forward / backward: HALF a wave per row of H = 256*V elements, each lane owning V runs of 8 consecutive elements, so that
// every access of the 16-bit rows is 16 bytes wide (512 contiguous bytes per half wave and instruction; the 8-byte form of
// rounds 1-2 ran at 0.50-0.60 of the HBM rate).  The embedding kernel keeps one wave per row: its rows are fp32 (16-byte accesses
// already).
#include "common.h"
#include "dropout.h"

namespace {

template <int V>
__device__ __forceinline__ void row_stats(const float (&x)[V][4], int H, float& mean, float& rstd, float eps) {
    float s = 0.f;
#pragma unroll
    for (int v = 0; v < V; ++v)
#pragma unroll
        for (int r = 0; r < 4; ++r) s += x[v][r];
    mean = wave_sum(s) / (float)H;
    float q = 0.f;
#pragma unroll
    for (int v = 0; v < V; ++v)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float d = x[v][r] - mean;
            q += d * d;
        }
    rstd = rsqrtf(wave_sum(q) / (float)H + eps);
}

// tnlrv3/modeling.py:153-178 (word + pos + type0 -> LN) fused with the mask of :446-454
template <int V, typename TokT>
__global__ __launch_bounds__(256) void embed_ln_kernel(const TokT* __restrict__ tok, const int32_t* __restrict__ nidx,
                                                       int64_t n_tok, int L,
                                                       const float* __restrict__ word, const float* __restrict__ pos,
                                                       const float* __restrict__ type0, const float* __restrict__ gamma,
                                                       const float* __restrict__ beta, float eps, bf16* __restrict__ out,
                                                       float* __restrict__ mask_add, TnrDrop drop,
                                                       const int32_t* __restrict__ pos_ids) {
    const int H = 256 * V;
    const int lane = threadIdx.x & 63;
    int64_t t = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (t >= n_tok) return;
    int64_t n = t / L;
    int i = (int)(t - n * L);
    const int64_t trow = nidx ? (int64_t)nidx[n] : n;       // news index -> row of the resident token table
    int64_t id = (int64_t)tok[trow * 2 * L + i];
    if (lane == 0) {
        const int Lr = (L + 31) & ~31;                       // mask rows are padded to a multiple of 32 keys
        int64_t mk = (int64_t)tok[trow * 2 * L + L + i];
        mask_add[n * Lr + i] = (1.0f - (float)mk) * -10000.0f;
        if (i == 0)
            for (int j = L; j < Lr; ++j) mask_add[n * Lr + j] = -1e30f;
    }
    // position row: the token's index (BERT / UniLM, tnlrv3/modeling.py:164-167), or a per-token id table laid out like the
    // token table (RoBERTa: cumulative count of non-pad tokens + padding_idx, PLM-NR's --model_type roberta)
    const int pi = pos_ids ? pos_ids[trow * L + i] : i;
    float x[V][4];
#pragma unroll
    for (int v = 0; v < V; ++v) {
        int c = v * 256 + lane * 4;
        f32x4 a = *(const f32x4*)(word + id * H + c);
        f32x4 b = *(const f32x4*)(pos + (int64_t)pi * H + c);
        f32x4 d = *(const f32x4*)(type0 + c);
#pragma unroll
        for (int r = 0; r < 4; ++r) x[v][r] = a[r] + b[r] + d[r];
    }
    float mean, rstd;
    row_stats<V>(x, H, mean, rstd, eps);
#pragma unroll
    for (int v = 0; v < V; ++v) {
        int c = v * 256 + lane * 4;
        f32x4 gm = *(const f32x4*)(gamma + c);
        f32x4 bt = *(const f32x4*)(beta + c);
        float dm[4] = {1.f, 1.f, 1.f, 1.f};
        if (drop.thresh) tnr_drop4(drop, (uint64_t)t * H + c, dm);          // tnlrv3/modeling.py:177
        bf16x4 o;
#pragma unroll
        for (int r = 0; r < 4; ++r) o[r] = (bf16)(((x[v][r] - mean) * rstd * gm[r] + bt[r]) * dm[r]);
        *(bf16x4*)(out + t * H + c) = o;
    }
}

// Backward of embed_ln_kernel (tnlrv3/modeling.py:153-178).  The forward saves nothing: x = word[id] + pos[pi] + type0 and the
// row statistics are recomputed exactly as it computes them (one wave per token, row_stats), the DROP_EMB mask of :177 is
// regenerated at element t * H + c.  With g = dy * mask * gamma:
//   dx = inv_scale * rstd * (g - mean(g) - xh * mean(g * xh))   fp32 rows: what the scatter / column sums of the tables add up
//   part[block] = [sum dy * mask * xh | sum dy * mask]           one row per block, at dy's (loss) scale, summed in a fixed order
// A block takes rows_per_block consecutive tokens (embwd_rows, common.h), four at a time.
template <int V, typename TokT>
__global__ __launch_bounds__(256) void embed_ln_bwd_kernel(const TokT* __restrict__ tok, const int32_t* __restrict__ nidx,
                                                           int64_t n_tok, int L, const bf16* __restrict__ dy,
                                                           const float* __restrict__ word, const float* __restrict__ pos,
                                                           const float* __restrict__ type0, const float* __restrict__ gamma,
                                                           float eps, float inv_scale, float* __restrict__ dx,
                                                           float* __restrict__ part, int rows_per_block, TnrDrop drop,
                                                           const int32_t* __restrict__ pos_ids) {
    const int H = 256 * V;
    __shared__ float red[4][2][256 * V];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    float gm[V][4], dg[V][4], db[V][4];
#pragma unroll
    for (int v = 0; v < V; ++v) {
        const f32x4 t0 = *(const f32x4*)(gamma + v * 256 + lane * 4);
#pragma unroll
        for (int r = 0; r < 4; ++r) { gm[v][r] = t0[r]; dg[v][r] = 0.f; db[v][r] = 0.f; }
    }
    for (int it = 0; it < rows_per_block / 4; ++it) {
        const int64_t t = (int64_t)blockIdx.x * rows_per_block + it * 4 + w;
        if (t >= n_tok) break;
        const int64_t n = t / L;
        const int i = (int)(t - n * L);
        const int64_t trow = nidx ? (int64_t)nidx[n] : n;
        const int64_t id = (int64_t)tok[trow * 2 * L + i];
        const int pi = pos_ids ? pos_ids[trow * L + i] : i;
        float x[V][4], g[V][4];
#pragma unroll
        for (int v = 0; v < V; ++v) {
            const int c = v * 256 + lane * 4;
            const f32x4 a = *(const f32x4*)(word + id * H + c);
            const f32x4 b = *(const f32x4*)(pos + (int64_t)pi * H + c);
            const f32x4 d = *(const f32x4*)(type0 + c);
#pragma unroll
            for (int r = 0; r < 4; ++r) x[v][r] = a[r] + b[r] + d[r];
        }
        float mean, rstd;
        row_stats<V>(x, H, mean, rstd, eps);
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int v = 0; v < V; ++v) {
            const int c = v * 256 + lane * 4;
            const bf16x4 d = *(const bf16x4*)(dy + t * H + c);
            float dm[4] = {1.f, 1.f, 1.f, 1.f};
            if (drop.thresh) tnr_drop4(drop, (uint64_t)t * H + c, dm);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float dyv = (float)d[r] * dm[r];
                x[v][r] = (x[v][r] - mean) * rstd;           // xh
                g[v][r] = dyv * gm[v][r];
                s1 += g[v][r];
                s2 += g[v][r] * x[v][r];
                dg[v][r] += dyv * x[v][r];
                db[v][r] += dyv;
            }
        }
        s1 = wave_sum(s1) / (float)H;
        s2 = wave_sum(s2) / (float)H;
        const float k = inv_scale * rstd;
#pragma unroll
        for (int v = 0; v < V; ++v) {
            f32x4 o;
#pragma unroll
            for (int r = 0; r < 4; ++r) o[r] = k * (g[v][r] - s1 - x[v][r] * s2);
            *(f32x4*)(dx + t * H + v * 256 + lane * 4) = o;
        }
    }
    // the four waves own the same columns: combined through LDS in wave order
#pragma unroll
    for (int v = 0; v < V; ++v)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            red[w][0][v * 256 + lane * 4 + r] = dg[v][r];
            red[w][1][v * 256 + lane * 4 + r] = db[v][r];
        }
    __syncthreads();
    for (int c = threadIdx.x; c < 2 * H; c += 256) {
        const int k = c / H, h = c - k * H;
        part[(int64_t)blockIdx.x * 2 * H + c] = (red[0][k][h] + red[1][k][h]) + (red[2][k][h] + red[3][k][h]);
    }
}

__device__ __forceinline__ float half_sum(float v) {      // over the 32 lanes of this lane's half wave
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

template <int V>
__global__ __launch_bounds__(256) void ln_fwd_kernel(const bf16* __restrict__ xin, const float* __restrict__ gamma,
                                                     const float* __restrict__ beta, float eps, bf16* __restrict__ y,
                                                     float* __restrict__ stats, int64_t M) {
    const int H = 256 * V;
    const int hl = threadIdx.x & 31;
    int64_t m = (int64_t)blockIdx.x * 8 + (threadIdx.x >> 5);
    if (m >= M) return;
    float x[V][8];
    float s = 0.f;
#pragma unroll
    for (int v = 0; v < V; ++v) {
        const bf16x8 a = *(const bf16x8*)(xin + m * H + v * 256 + hl * 8);
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            x[v][r] = (float)a[r];
            s += x[v][r];
        }
    }
    const float mean = half_sum(s) / (float)H;
    float q = 0.f;
#pragma unroll
    for (int v = 0; v < V; ++v)
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const float d = x[v][r] - mean;
            q += d * d;
        }
    const float rstd = rsqrtf(half_sum(q) / (float)H + eps);
    if (stats && hl == 0) {
        stats[m * 2] = mean;
        stats[m * 2 + 1] = rstd;
    }
#pragma unroll
    for (int v = 0; v < V; ++v) {
        const int c = v * 256 + hl * 8;
        const f32x4 g0 = *(const f32x4*)(gamma + c), g1 = *(const f32x4*)(gamma + c + 4);
        const f32x4 b0 = *(const f32x4*)(beta + c), b1 = *(const f32x4*)(beta + c + 4);
        bf16x8 o;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            o[r] = (bf16)((x[v][r] - mean) * rstd * g0[r] + b0[r]);
            o[4 + r] = (bf16)((x[v][4 + r] - mean) * rstd * g1[r] + b1[r]);
        }
        *(bf16x8*)(y + m * H + c) = o;
    }
}

// dx = rstd * (dxh - mean(dxh) - xh * mean(dxh*xh)), dxh = dy*gamma ; per-block partial dgamma/dbeta (rows per block: lnb_rows, common.h)
template <int V>
__global__ __launch_bounds__(256) void ln_bwd_kernel(const bf16* __restrict__ dy, const bf16* __restrict__ xin,
                                                     const float* __restrict__ stats, const float* __restrict__ gamma,
                                                     bf16* __restrict__ dx, float* __restrict__ part, int64_t M,
                                                     int rows_per_block, bf16* __restrict__ dxm, TnrDrop drop) {
    const int H = 256 * V;
    __shared__ float red[4][3][256 * V];
    const int lane = threadIdx.x & 63, hl = lane & 31, w = threadIdx.x >> 6, hw = threadIdx.x >> 5;
    float gm[V][8], dg[V][8], db[V][8], dxs[V][8];
#pragma unroll
    for (int v = 0; v < V; ++v) {
        const f32x4 t0 = *(const f32x4*)(gamma + v * 256 + hl * 8), t1 = *(const f32x4*)(gamma + v * 256 + hl * 8 + 4);
#pragma unroll
        for (int r = 0; r < 4; ++r) { gm[v][r] = t0[r]; gm[v][4 + r] = t1[r]; }
#pragma unroll
        for (int r = 0; r < 8; ++r) { dg[v][r] = 0.f; db[v][r] = 0.f; dxs[v][r] = 0.f; }
    }
    for (int it = 0; it < rows_per_block / 8; ++it) {
        const int64_t m = (int64_t)blockIdx.x * rows_per_block + it * 8 + hw;
        if (m >= M) break;
        const float mean = stats[m * 2], rstd = stats[m * 2 + 1];
        float xh[V][8], g[V][8];
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int v = 0; v < V; ++v) {
            const bf16x8 a = *(const bf16x8*)(xin + m * H + v * 256 + hl * 8);
            const bf16x8 d = *(const bf16x8*)(dy + m * H + v * 256 + hl * 8);
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                const float dyv = (float)d[r];
                xh[v][r] = ((float)a[r] - mean) * rstd;
                g[v][r] = dyv * gm[v][r];
                s1 += g[v][r];
                s2 += g[v][r] * xh[v][r];
                dg[v][r] += dyv * xh[v][r];
                db[v][r] += dyv;
            }
        }
        s1 = half_sum(s1) / (float)H;
        s2 = half_sum(s2) / (float)H;
#pragma unroll
        for (int v = 0; v < V; ++v) {
            bf16x8 o;
            if (dxm) {
                // the Linear in front of this LayerNorm was followed by dropout (BertSelfOutput / BertOutput): its output
                // gradient is dx * mask / (1 - p) (second output, what its wgrad / dgrad / bias gradient consume), the
                // residual branch takes dx itself
                float dm[8];
                uint32_t dc;
                const uint32_t mr = tnr_drop_row(drop, (uint32_t)m, dc);     // rows behind a split: the tail pass's own mask
                tnr_drop8(drop, dc, ((uint64_t)mr * H + v * 256 + hl * 8) >> 3, dm);
                bf16x8 om;
#pragma unroll
                for (int r = 0; r < 8; ++r) {
                    const float t = rstd * (g[v][r] - s1 - xh[v][r] * s2);
                    o[r] = (bf16)t;
                    om[r] = (bf16)(t * dm[r]);
                    dxs[v][r] += (float)om[r];
                }
                *(bf16x8*)(dxm + m * H + v * 256 + hl * 8) = om;
            } else {
#pragma unroll
                for (int r = 0; r < 8; ++r) {
                    o[r] = (bf16)(rstd * (g[v][r] - s1 - xh[v][r] * s2));
                    dxs[v][r] += (float)o[r];          // the rounded value the wgrad kernels will see
                }
            }
            *(bf16x8*)(dx + m * H + v * 256 + hl * 8) = o;
        }
    }
    if (part == nullptr) return;
    // the two half waves of a wave own the same columns: combine them, then the four waves through LDS (fixed order)
#pragma unroll
    for (int v = 0; v < V; ++v)
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const float a = dg[v][r] + __shfl_xor(dg[v][r], 32, 64);
            const float b = db[v][r] + __shfl_xor(db[v][r], 32, 64);
            const float c = dxs[v][r] + __shfl_xor(dxs[v][r], 32, 64);
            if (lane < 32) {
                red[w][0][v * 256 + hl * 8 + r] = a;
                red[w][1][v * 256 + hl * 8 + r] = b;
                red[w][2][v * 256 + hl * 8 + r] = c;
            }
        }
    __syncthreads();
    for (int c = threadIdx.x; c < 3 * H; c += 256) {
        int k = c / H, h = c - k * H;
        part[(int64_t)blockIdx.x * 3 * H + c] = red[0][k][h] + red[1][k][h] + red[2][k][h] + red[3][k][h];
    }
}

__global__ void cast_f2b_kernel(const float* __restrict__ s, bf16* __restrict__ d, int64_t n) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) d[i] = (bf16)s[i];
}
__global__ void cast_b2f_kernel(const bf16* __restrict__ s, float* __restrict__ d, int64_t n) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) d[i] = (float)s[i];
}


// NewsEncoder pooling other than 'att' (model_bert.py:130-135): 'cls' = hidden state of token 0, otherwise the mean
// over ALL L positions (padding included, as torch.mean(word_vecs, dim=1)).  One workgroup per sequence.
__global__ __launch_bounds__(256) void pool_fwd_kernel(const bf16* __restrict__ y, float* __restrict__ nv, int L, int H,
                                                       int mean) {
    const int64_t n = blockIdx.x;
    for (int c = threadIdx.x * 4; c < H; c += 1024) {
        f32x4 a = (f32x4){0.f, 0.f, 0.f, 0.f};
        const int rows = mean ? L : 1;
        for (int i = 0; i < rows; ++i) {
            bf16x4 v = *(const bf16x4*)(y + (n * L + i) * H + c);
            a += (f32x4){(float)v[0], (float)v[1], (float)v[2], (float)v[3]};
        }
        if (mean) a *= 1.0f / (float)L;
        *(f32x4*)(nv + n * H + c) = a;
    }
}

__global__ __launch_bounds__(256) void pool_bwd_kernel(const float* __restrict__ dnv, bf16* __restrict__ dy, int L, int H,
                                                       int mean) {
    const int64_t n = blockIdx.x;
    for (int c = threadIdx.x * 4; c < H; c += 1024) {
        f32x4 g = *(const f32x4*)(dnv + n * H + c);
        if (mean) g *= 1.0f / (float)L;
        bf16x4 o = (bf16x4){(bf16)g[0], (bf16)g[1], (bf16)g[2], (bf16)g[3]};
        bf16x4 zero = (bf16x4){(bf16)0.f, (bf16)0.f, (bf16)0.f, (bf16)0.f};
        for (int i = 0; i < L; ++i) *(bf16x4*)(dy + (n * L + i) * H + c) = (mean || i == 0) ? o : zero;
    }
}

// the 16-bit copies (row-major and transposed) of the fp32 weights the GEMMs read, refreshed after every optimiser step:
// one workgroup per 32x32 tile of some weight matrix (descriptor table on device)
__global__ __launch_bounds__(256) void refresh_kernel(const int64_t* __restrict__ desc, int n_desc,
                                                      const int64_t* __restrict__ tile_start) {
    __shared__ float t[32][33];
    int64_t tile = blockIdx.x;
    int di = 0;
    while (di + 1 < n_desc && tile >= tile_start[di + 1]) ++di;
    const int64_t* d = desc + (int64_t)di * 8;
    const float* src = (const float*)d[0];
    const int64_t rows = d[1], cols = d[2];
    bf16* dst = (bf16*)d[3];
    const int64_t ld = d[4];
    bf16* dstT = (bf16*)d[5];
    const int64_t ldT = d[6];
    const int64_t local = tile - tile_start[di];
    const int64_t tcols = (cols + 31) / 32;
    const int64_t r0 = (local / tcols) * 32, c0 = (local % tcols) * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;    // 32 x 8
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        int64_t r = r0 + ty + 8 * k, c = c0 + tx;
        float v = (r < rows && c < cols) ? src[r * cols + c] : 0.f;
        t[ty + 8 * k][tx] = v;
        if (dst && r < rows && c < cols) dst[r * ld + c] = (bf16)v;
    }
    __syncthreads();
    if (dstT) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            int64_t c = c0 + ty + 8 * k, r = r0 + tx;
            if (r < rows && c < cols) dstT[c * ldT + r] = (bf16)t[tx][ty + 8 * k];
        }
    }
}

}  // namespace

extern "C" int TNR_NAME(tnr_embed_ln_fwd_do)(const int64_t* tok, int64_t n_seq, int L, int H, const float* word, const float* pos,
                                   const float* type0, const float* gamma, const float* beta, float eps, void* out,
                                   float* mask_add, const tnr_dropout_t* drop, const int32_t* pos_ids, void* stream) {
    TnrDrop dd;
    if (int rc = tnr_make_drop(drop, &dd, "tnr_embed_ln_fwd")) return rc;
    TNR_CHECK_ARG(tok && word && pos && type0 && gamma && beta && out && mask_add, "tnr_embed_ln_fwd: null pointer");
    TNR_CHECK_ARG(L >= 1 && L <= 512 && n_seq >= 1, "tnr_embed_ln_fwd: need 1<=L<=512");
    TNR_CHECK_ARG(H == 768 || H == 256 || H == 512 || H == 1024, "tnr_embed_ln_fwd: H must be 256/512/768/1024");
    int64_t n_tok = n_seq * L;
    dim3 grid((unsigned)((n_tok + 3) / 4)), blk(256);
    hipStream_t st = (hipStream_t)stream;
#define LAUNCH(V) hipLaunchKernelGGL((embed_ln_kernel<V, int64_t>), grid, blk, 0, st, tok, (const int32_t*)nullptr, n_tok, L, word, pos, type0, gamma, beta, eps, (bf16*)out, mask_add, dd, pos_ids)
    switch (H / 256) { case 1: LAUNCH(1); break; case 2: LAUNCH(2); break; case 3: LAUNCH(3); break; default: LAUNCH(4); }
#undef LAUNCH
    TNR_CHECK_LAUNCH("tnr_embed_ln_fwd");
    return TNR_OK;
}
extern "C" int TNR_NAME(tnr_embed_ln_fwd)(const int64_t* tok, int64_t n_seq, int L, int H, const float* word, const float* pos,
                                const float* type0, const float* gamma, const float* beta, float eps, void* out,
                                float* mask_add, void* stream) {
    return TNR_NAME(tnr_embed_ln_fwd_do)(tok, n_seq, L, H, word, pos, type0, gamma, beta, eps, out, mask_add, nullptr, nullptr, stream);
}

extern "C" int TNR_NAME(tnr_embed_ln_fwd_indexed_do)(const int32_t* news_combined, const int32_t* nidx, int64_t n_seq, int L, int H,
                                           const float* word, const float* pos, const float* type0, const float* gamma,
                                           const float* beta, float eps, void* out, float* mask_add,
                                           const tnr_dropout_t* drop, const int32_t* pos_ids, void* stream) {
    TnrDrop dd;
    if (int rc = tnr_make_drop(drop, &dd, "tnr_embed_ln_fwd_indexed")) return rc;
    TNR_CHECK_ARG(news_combined && nidx && word && pos && type0 && gamma && beta && out && mask_add,
                  "tnr_embed_ln_fwd_indexed: null pointer");
    TNR_CHECK_ARG(L >= 1 && L <= 512 && n_seq >= 1, "tnr_embed_ln_fwd_indexed: need 1<=L<=512");
    TNR_CHECK_ARG(H == 768 || H == 256 || H == 512 || H == 1024, "tnr_embed_ln_fwd_indexed: H must be 256/512/768/1024");
    int64_t n_tok = n_seq * L;
    dim3 grid((unsigned)((n_tok + 3) / 4)), blk(256);
    hipStream_t st = (hipStream_t)stream;
#define LAUNCH(V) hipLaunchKernelGGL((embed_ln_kernel<V, int32_t>), grid, blk, 0, st, news_combined, nidx, n_tok, L, word, pos, type0, gamma, beta, eps, (bf16*)out, mask_add, dd, pos_ids)
    switch (H / 256) { case 1: LAUNCH(1); break; case 2: LAUNCH(2); break; case 3: LAUNCH(3); break; default: LAUNCH(4); }
#undef LAUNCH
    TNR_CHECK_LAUNCH("tnr_embed_ln_fwd_indexed");
    return TNR_OK;
}
extern "C" int TNR_NAME(tnr_embed_ln_fwd_indexed)(const int32_t* news_combined, const int32_t* nidx, int64_t n_seq, int L, int H,
                                        const float* word, const float* pos, const float* type0, const float* gamma,
                                        const float* beta, float eps, void* out, float* mask_add, void* stream) {
    return TNR_NAME(tnr_embed_ln_fwd_indexed_do)(news_combined, nidx, n_seq, L, H, word, pos, type0, gamma, beta, eps, out, mask_add,
                                                 nullptr, nullptr, stream);
}

extern "C" int TNR_NAME(tnr_embed_ln_bwd)(const int64_t* tok, int64_t n_seq, int L, int H, const void* dy, const float* word,
                                const float* pos, const float* type0, const float* gamma, float eps, float inv_scale, float* dx,
                                float* part, const tnr_dropout_t* drop, const int32_t* pos_ids, void* stream) {
    TnrDrop dd;
    if (int rc = tnr_make_drop(drop, &dd, "tnr_embed_ln_bwd")) return rc;
    TNR_CHECK_ARG(tok && dy && word && pos && type0 && gamma && dx && part, "tnr_embed_ln_bwd: null pointer");
    TNR_CHECK_ARG(L >= 1 && L <= 512 && n_seq >= 1, "tnr_embed_ln_bwd: need 1<=L<=512");
    TNR_CHECK_ARG(H == 768 || H == 256 || H == 512 || H == 1024, "tnr_embed_ln_bwd: H must be 256/512/768/1024");
    const int64_t n_tok = n_seq * L;
    const int rows = embwd_rows(n_tok);
    dim3 grid((unsigned)embwd_blocks(n_tok)), blk(256);
    hipStream_t st = (hipStream_t)stream;
#define LAUNCH(V) hipLaunchKernelGGL((embed_ln_bwd_kernel<V, int64_t>), grid, blk, 0, st, tok, (const int32_t*)nullptr, n_tok, L, (const bf16*)dy, word, pos, type0, gamma, eps, inv_scale, dx, part, rows, dd, pos_ids)
    switch (H / 256) { case 1: LAUNCH(1); break; case 2: LAUNCH(2); break; case 3: LAUNCH(3); break; default: LAUNCH(4); }
#undef LAUNCH
    TNR_CHECK_LAUNCH("tnr_embed_ln_bwd");
    return TNR_OK;
}

extern "C" int TNR_NAME(tnr_embed_ln_bwd_indexed)(const int32_t* news_combined, const int32_t* nidx, int64_t n_seq, int L, int H,
                                        const void* dy, const float* word, const float* pos, const float* type0,
                                        const float* gamma, float eps, float inv_scale, float* dx, float* part,
                                        const tnr_dropout_t* drop, const int32_t* pos_ids, void* stream) {
    TnrDrop dd;
    if (int rc = tnr_make_drop(drop, &dd, "tnr_embed_ln_bwd_indexed")) return rc;
    TNR_CHECK_ARG(news_combined && nidx && dy && word && pos && type0 && gamma && dx && part, "tnr_embed_ln_bwd_indexed: null pointer");
    TNR_CHECK_ARG(L >= 1 && L <= 512 && n_seq >= 1, "tnr_embed_ln_bwd_indexed: need 1<=L<=512");
    TNR_CHECK_ARG(H == 768 || H == 256 || H == 512 || H == 1024, "tnr_embed_ln_bwd_indexed: H must be 256/512/768/1024");
    const int64_t n_tok = n_seq * L;
    const int rows = embwd_rows(n_tok);
    dim3 grid((unsigned)embwd_blocks(n_tok)), blk(256);
    hipStream_t st = (hipStream_t)stream;
#define LAUNCH(V) hipLaunchKernelGGL((embed_ln_bwd_kernel<V, int32_t>), grid, blk, 0, st, news_combined, nidx, n_tok, L, (const bf16*)dy, word, pos, type0, gamma, eps, inv_scale, dx, part, rows, dd, pos_ids)
    switch (H / 256) { case 1: LAUNCH(1); break; case 2: LAUNCH(2); break; case 3: LAUNCH(3); break; default: LAUNCH(4); }
#undef LAUNCH
    TNR_CHECK_LAUNCH("tnr_embed_ln_bwd_indexed");
    return TNR_OK;
}

extern "C" int TNR_NAME(tnr_pool_fwd)(const void* y, float* nv, int64_t n_seq, int L, int H, int mean, void* stream) {
    TNR_CHECK_ARG(y && nv && n_seq >= 1 && L >= 1 && H >= 4 && (H % 4) == 0, "tnr_pool_fwd: bad argument");
    hipLaunchKernelGGL(pool_fwd_kernel, dim3((unsigned)n_seq), dim3(256), 0, (hipStream_t)stream, (const bf16*)y, nv, L, H,
                       mean);
    TNR_CHECK_LAUNCH("tnr_pool_fwd");
    return TNR_OK;
}

extern "C" int TNR_NAME(tnr_pool_bwd)(const float* dnv, void* dy, int64_t n_seq, int L, int H, int mean, void* stream) {
    TNR_CHECK_ARG(dnv && dy && n_seq >= 1 && L >= 1 && H >= 4 && (H % 4) == 0, "tnr_pool_bwd: bad argument");
    hipLaunchKernelGGL(pool_bwd_kernel, dim3((unsigned)n_seq), dim3(256), 0, (hipStream_t)stream, dnv, (bf16*)dy, L, H, mean);
    TNR_CHECK_LAUNCH("tnr_pool_bwd");
    return TNR_OK;
}

extern "C" int TNR_NAME(tnr_ln_fwd)(const void* x, const float* gamma, const float* beta, float eps, void* y, float* stats,
                          int64_t M, int H, void* stream) {
    TNR_CHECK_ARG(x && gamma && beta && y && M >= 1, "tnr_ln_fwd: null pointer");
    TNR_CHECK_ARG(H == 768 || H == 256 || H == 512 || H == 1024, "tnr_ln_fwd: H must be 256/512/768/1024");
    dim3 grid((unsigned)((M + 7) / 8)), blk(256);        // half a wave per row
    hipStream_t st = (hipStream_t)stream;
#define LAUNCH(V) hipLaunchKernelGGL(ln_fwd_kernel<V>, grid, blk, 0, st, (const bf16*)x, gamma, beta, eps, (bf16*)y, stats, M)
    switch (H / 256) { case 1: LAUNCH(1); break; case 2: LAUNCH(2); break; case 3: LAUNCH(3); break; default: LAUNCH(4); }
#undef LAUNCH
    TNR_CHECK_LAUNCH("tnr_ln_fwd");
    return TNR_OK;
}

extern "C" int TNR_NAME(tnr_ln_bwd_do)(const void* dy, const void* x, const float* stats, const float* gamma, void* dx,
                             float* dgamma, float* dbeta, float* dxsum, float* part, int64_t M, int H, void* dxm,
                             const tnr_dropout_t* drop, void* stream) {
    return TNR_NAME(tnr_ln_bwd_do_split)(dy, x, stats, gamma, dx, dgamma, dbeta, dxsum, part, M, H, dxm, drop, nullptr, M, stream);
}
extern "C" int TNR_NAME(tnr_ln_bwd_do_split)(const void* dy, const void* x, const float* stats, const float* gamma, void* dx,
                                   float* dgamma, float* dbeta, float* dxsum, float* part, int64_t M, int H, void* dxm,
                                   const tnr_dropout_t* drop, const tnr_dropout_t* drop_tail, int64_t split_row, void* stream) {
    // dgamma == dbeta == dxsum == NULL with part != NULL: partials only, the caller reduces them (tnr_reduce_multi)
    TnrDrop dd;
    if (int rc = tnr_make_drop_split(drop, drop_tail, split_row, M, &dd, "tnr_ln_bwd")) return rc;
    TNR_CHECK_ARG(dxm || !dd.thresh, "tnr_ln_bwd: an active dropout site needs the masked second output");
    TNR_CHECK_ARG(dy && x && stats && gamma && dx && M >= 1, "tnr_ln_bwd: null pointer");
    TNR_CHECK_ARG(H == 768 || H == 256 || H == 512 || H == 1024, "tnr_ln_bwd: H must be 256/512/768/1024");
    TNR_CHECK_ARG(!(dgamma || dbeta || dxsum) || part, "tnr_ln_bwd: part workspace required for dgamma/dbeta/dxsum");
    int64_t nblk = lnb_blocks(M);
    const int rows = lnb_rows(M);
    dim3 grid((unsigned)nblk), blk(256);
    hipStream_t st = (hipStream_t)stream;
    float* p = part;
#define LAUNCH(V) hipLaunchKernelGGL(ln_bwd_kernel<V>, grid, blk, 0, st, (const bf16*)dy, (const bf16*)x, stats, gamma, (bf16*)dx, p, M, rows, (bf16*)dxm, dd)
    switch (H / 256) { case 1: LAUNCH(1); break; case 2: LAUNCH(2); break; case 3: LAUNCH(3); break; default: LAUNCH(4); }
#undef LAUNCH
    TNR_CHECK_LAUNCH("tnr_ln_bwd");
    if (dgamma && dbeta == dgamma + H) {       // adjacent in the flat gradient buffer: one reduction
        int rc = tnr_reduce_rows(part, nblk, 3 * H, 2 * H, dgamma, 0, stream); if (rc) return rc;
    } else {
        if (dgamma) { int rc = tnr_reduce_rows(part, nblk, 3 * H, H, dgamma, 0, stream); if (rc) return rc; }
        if (dbeta) { int rc = tnr_reduce_rows(part + H, nblk, 3 * H, H, dbeta, 0, stream); if (rc) return rc; }
    }
    if (dxsum) { int rc = tnr_reduce_rows(part + 2 * H, nblk, 3 * H, H, dxsum, 0, stream); if (rc) return rc; }
    return TNR_OK;
}
extern "C" int TNR_NAME(tnr_ln_bwd)(const void* dy, const void* x, const float* stats, const float* gamma, void* dx,
                          float* dgamma, float* dbeta, float* dxsum, float* part, int64_t M, int H, void* stream) {
    return TNR_NAME(tnr_ln_bwd_do)(dy, x, stats, gamma, dx, dgamma, dbeta, dxsum, part, M, H, nullptr, nullptr, stream);
}

extern "C" int TNR_NAME(tnr_colsum_batched)(const void* X, int64_t ldx, int64_t sX, int dtype, int64_t M, int64_t N, int batch,
                                  float* out, float* part, int accumulate, void* stream) {
    TNR_CHECK_ARG(X && out && part && M >= 1 && N >= 4 && (N % 4) == 0 && (ldx % 4) == 0 && batch >= 1, "tnr_colsum: bad argument");
    TNR_CHECK_ARG(dtype == TNR_BF16 || dtype == TNR_F16 || dtype == TNR_F32, "tnr_colsum: dtype");
    const int rpb = cs_rows(M);
    int64_t nby = (M + rpb - 1) / rpb;
    dim3 grid((unsigned)((N + 255) / 256), (unsigned)nby, (unsigned)batch), blk(256);
    // partials laid out (nby, batch, N) so that ONE row reduction yields out (batch, N)
    if (dtype != TNR_F32)      // the 16-bit type of this build
        hipLaunchKernelGGL(colsum_kernel<bf16>, grid, blk, 0, (hipStream_t)stream, (const bf16*)X, ldx, M, N, part, sX, N, rpb);
    else
        colsum_f32_launch(grid, (const float*)X, ldx, M, N, part, sX, rpb, (hipStream_t)stream);
    TNR_CHECK_LAUNCH("tnr_colsum");
    return tnr_reduce_rows(part, nby, (int64_t)batch * N, (int64_t)batch * N, out, accumulate, stream);
}

extern "C" int TNR_NAME(tnr_colsum)(const void* X, int64_t ldx, int dtype, int64_t M, int64_t N, float* out, float* part,
                          int accumulate, void* stream) {
    return TNR_NAME(tnr_colsum_batched)(X, ldx, 0, dtype, M, N, 1, out, part, accumulate, stream);
}

extern "C" int TNR_NAME(tnr_cast_f32_to_bf16)(const float* src, void* dst, int64_t n, void* stream) {
    TNR_CHECK_ARG(src && dst && n >= 1, "tnr_cast_f32_to_bf16: bad argument");
    hipLaunchKernelGGL(cast_f2b_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, src, (bf16*)dst, n);
    TNR_CHECK_LAUNCH("tnr_cast_f32_to_bf16");
    return TNR_OK;
}
extern "C" int TNR_NAME(tnr_cast_bf16_to_f32)(const void* src, float* dst, int64_t n, void* stream) {
    TNR_CHECK_ARG(src && dst && n >= 1, "tnr_cast_bf16_to_f32: bad argument");
    hipLaunchKernelGGL(cast_b2f_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const bf16*)src, dst, n);
    TNR_CHECK_LAUNCH("tnr_cast_bf16_to_f32");
    return TNR_OK;
}

extern "C" int TNR_NAME(tnr_refresh_shadows)(const int64_t* desc, int n_desc, int64_t total_tiles, const int64_t* tile_start,
                                   void* stream) {
    TNR_CHECK_ARG(desc && tile_start && n_desc >= 1 && total_tiles >= 1, "tnr_refresh_shadows: bad argument");
    hipLaunchKernelGGL(refresh_kernel, dim3((unsigned)total_tiles), dim3(256), 0, (hipStream_t)stream, desc, n_desc,
                       tile_start);
    TNR_CHECK_LAUNCH("tnr_refresh_shadows");
    return TNR_OK;
}
