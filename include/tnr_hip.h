/* libtnr_hip.so -- C ABI of the MI355X (gfx950) hot path of Tiny-NewsRec training.
 *
 * The reference has no FFI layer: the path sits behind Python modules and every
 * device op is a stock ATen kernel.  Each entry point
 * below replaces the ATen ops the cited reference lines launch.  Citations are
 * /root/reference/Tiny-NewsRec/<file>:<line>.
 *
 * Conventions:
 *   - plain pointers + explicit sizes; every tensor pointer is DEVICE memory
 *     owned by the caller (PyTorch allocator), including workspaces;
 *   - every call is asynchronous on `stream` (a hipStream_t passed as void*);
 *   - return 0 on success, a negative TNR_E* code otherwise; tnr_last_error()
 *     returns a thread-local message; no C++ exception crosses the boundary;
 *   - the library never calls hipSetDevice / hipDeviceSynchronize / hipStreamSynchronize: the caller's current device
 *     rules and nothing ever blocks the host;
 *   - device state kept by the library: ONE thing, the tile-queue counters of the persistent GEMMs (see
 *     tnr_gemm_queue_reset below); host state: the process-wide GEMM option block (tnr_gemm_set_option), the buffer pointer
 *     of tnr_gemm_clock_stamps and the run-time binding of RCCL (tnr_comm_*); everything else lives in caller-owned buffers;
 *   - 16-bit activations are bf16 (TNR_BF16); "ld" arguments are row strides in
 *     ELEMENTS; row-major everywhere.
 */
#ifndef TNR_HIP_H
#define TNR_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TNR_OK 0
#define TNR_EINVAL (-1)      /* bad shape / alignment / null pointer */
#define TNR_EUNSUPPORTED (-2)
#define TNR_ELAUNCH (-3)     /* hipGetLastError() after a launch */

#define TNR_BF16 0
#define TNR_F16 1            /* IEEE half: the *_f16 entry points */
#define TNR_F32 2

/* gemm epilogue flags */
#define TNR_EPI_BIAS 1       /* + bias[n] (fp32) */
#define TNR_EPI_GELU 2       /* erf-GELU (transformers BertIntermediate, call site tnlrv3/modeling.py:305) */
#define TNR_EPI_TANH 4       /* model_bert.py:25 */
#define TNR_EPI_RES 8        /* + res[m,n] (bf16) : BertSelfOutput/BertOutput residual, tnlrv3/modeling.py:287,306 */
#define TNR_EPI_MULDGELU 16  /* * gelu'(aux[m,n])  : backward of TNR_EPI_GELU */
#define TNR_EPI_OUTF32 32    /* C is fp32 instead of bf16 */
#define TNR_EPI_AUXOUT 64    /* also store the pre-activation (acc+bias) to aux (bf16) */
#define TNR_EPI_COLSUM 128   /* tnr_gemm_nt_ex: also emit per-64-row-strip column sums of the bf16 output (bias grads) */
#define TNR_EPI_DROPOUT 256  /* internal: set by tnr_gemm_nt_do when a dropout site is passed (never by the caller) */

/* Dropout site for the *_do entry points (train-mode semantics of the stage-0 / stage-1 notebooks, which call .train():
 * Post-train_KD.ipynb cell 19, Domian-specific_Post-train.ipynb cell 16; sites tnlrv3/modeling.py:177, 224 and
 * BertSelfOutput / BertOutput at :287, :306).  A host struct, read at launch; NULL or p <= 0 = no dropout (bit-identical to
 * the entry point without the suffix).  Masks are counter-based (Philox4x32-10, csrc/dropout.h): nothing is stored, the
 * backward entry points regenerate them from the same (seed, site, call). */
typedef struct tnr_dropout {
    uint64_t seed;   /* run seed = Philox key */
    uint32_t site;   /* kind | layer << 8 ; kinds: 0 embeddings, 1 attention probabilities, 2 attention-output dense, 3 FFN-output dense */
    uint32_t call;   /* number of the forward pass (distinct per encoder pass and step) */
    double p;        /* drop probability ; kept elements are scaled by 1 / (1 - p) */
} tnr_dropout_t;

int tnr_version(void);
const char* tnr_last_error(void);

/* Every entry point is a single-device operation on the stream passed last, except the collectives tnr_comm_* at the end of
 * this file (the gradient exchange of the data-parallel step: RCCL behind a communicator the caller creates and owns); the
 * only per-(device, stream) state the library keeps is the GEMMs' tile-queue counter table described at tnr_gemm_queue_reset. */

/* ---- encoder --------------------------------------------------------------------------------- */

/* relative_position_bucket + one_hot + Linear(32->A) hoisted to one (A,32,32) fp32 table
 * (tnlrv3/modeling.py:345-373, 458-463).  weight (A,32) fp32.  Entries with i>=L or j>=L are 0.
 * In general the table is (A, Lr, Lr) with Lr = roundup(L, 32), L <= 512. */
int tnr_relpos_table(const float* weight, int A, int L, float* table, void* stream);

/* BertEmbeddings.forward (tnlrv3/modeling.py:153-178) + extended mask (:446-454), reading the padded
 * token batch directly: tok = (N, 2L) int64 rows [ids | mask] (model_bert.py:124-127).
 * out (N*L, H) bf16 ; mask_add (N,Lr) fp32 = (1-mask)*-10000, and -inf-like (-1e30) for j>=L ; Lr = roundup(L,32). */
int tnr_embed_ln_fwd(const int64_t* tok, int64_t n_seq, int L, int H, const float* word, const float* pos,
                     const float* type0, const float* gamma, const float* beta, float eps,
                     void* out, float* mask_add, void* stream);

/* Same, with the token rows gathered on the device: news_combined (n_news+1, 2L) int32 is the resident
 * table of preprocess.py:48-66 / run.py:53 and nidx (N) int32 the news indices of dataloader.py:129-138,
 * so only indices cross PCIe per step (the reference ships the gathered int64 rows, dataloader.py:152-154). */
int tnr_embed_ln_fwd_indexed(const int32_t* news_combined, const int32_t* nidx, int64_t n_seq, int L, int H,
                             const float* word, const float* pos, const float* type0, const float* gamma,
                             const float* beta, float eps, void* out, float* mask_add, void* stream);

/* Backward of the two forms above (BertEmbeddings.forward, tnlrv3/modeling.py:153-178; word table with padding_idx = 0, :138),
 * same token addressing; pos_ids (nullable) and drop (nullable, the DROP_EMB site) as in tnr_embed_ln_fwd_do.  The forward saves
 * nothing: x = word[id] + pos[pi] + type0 and its row statistics are recomputed in fp32 exactly as the forward computes them, the
 * dropout mask is regenerated.  dy (N*L, H) 16-bit = gradient w.r.t. the embedding output at the caller's loss scale.  With
 * g = dy * mask * gamma:
 *   dx (N*L, H) FP32 = inv_scale * rstd * (g - mean(g) - xh * mean(g * xh))      the true gradient of every token's summed row:
 *        the word / position / type tables' gradients are sums of its rows (tnr_scatter_sum_rows, tnr_colsum)
 *   part (nblk, 2H) fp32 = per-block [dgamma | dbeta] partial sums AT dy's SCALE (inv_scale is not applied: the reduction
 *        carries it, tnr_reduce_multi's descriptor scale), for tnr_reduce_rows / tnr_reduce_multi; fixed order.
 * H = 256 V, V = 1..4.  Token ids must be rows of `word`, position ids rows of `pos` (as in the forward). */
int tnr_embed_ln_bwd(const int64_t* tok, int64_t n_seq, int L, int H, const void* dy, const float* word, const float* pos,
                     const float* type0, const float* gamma, float eps, float inv_scale, float* dx, float* part,
                     const tnr_dropout_t* drop, const int32_t* pos_ids, void* stream);
int tnr_embed_ln_bwd_indexed(const int32_t* news_combined, const int32_t* nidx, int64_t n_seq, int L, int H, const void* dy,
                             const float* word, const float* pos, const float* type0, const float* gamma, float eps,
                             float inv_scale, float* dx, float* part, const tnr_dropout_t* drop, const int32_t* pos_ids,
                             void* stream);
int64_t tnr_embed_ln_bwd_part_elems(int64_t n_tok, int H);   /* workspace good for every token count <= n_tok */
int64_t tnr_embed_ln_bwd_blocks(int64_t n_tok);              /* partial rows (nblk) written for exactly n_tok tokens */

/* C[M,N] = epilogue(A[M,K] . B[N,K]^T).  bf16 operands, fp32 MFMA accumulation.
 * Forward Linear (tnlrv3/modeling.py:236-248, transformers BertSelfOutput/BertIntermediate/BertOutput),
 * and its dgrad when B is the transposed weight copy.  N % 128 == 0, K % 64 == 0, any M >= 1.
 * Only rows [0, M) of A, res and aux are ever used (a row tile that hangs over M re-reads row M - 1; what lies behind it in the
 * buffers is the caller's and may hold anything), and only rows [0, M) x columns [0, N) of C and of the TNR_EPI_AUXOUT output are
 * written: with a leading dimension above the width the gap columns keep their contents, in the operands they are never read.
 * Streams and threads: every entry point enqueues on `stream` and returns; calls may come from any thread.  The
 * persistent 256-column kernel hands its tiles out from a small counter block the library keeps per (device, stream) and
 * that the last workgroup of a launch zeroes again - launches of one stream are ordered, so each finds it zeroed; launches
 * on different streams use different blocks and may overlap (e.g. a collective on another stream: the workgroups that do
 * get a CU pull the tiles of those that do not). */
int tnr_gemm_nt(const void* A, int64_t lda, const void* B, int64_t ldb, void* C, int64_t ldc,
                int64_t M, int64_t N, int64_t K, const float* bias, const void* res, int64_t ldres,
                void* aux, int64_t ldaux, int flags, void* stream);

/* Same with an extra output for TNR_EPI_COLSUM: colsum_part (tnr_gemm_colsum_rows(M), N) fp32 whose rows sum
 * (tnr_reduce_rows) to the column sums of C -- the bias gradient of the Linear whose dgrad this GEMM is. */
int tnr_gemm_nt_ex(const void* A, int64_t lda, const void* B, int64_t ldb, void* C, int64_t ldc,
                   int64_t M, int64_t N, int64_t K, const float* bias, const void* res, int64_t ldres,
                   void* aux, int64_t ldaux, int flags, float* colsum_part, void* stream);
int64_t tnr_gemm_colsum_rows(int64_t M);

/* Debug / test hooks.  tnr_gemm_nt_route: which kernel tnr_gemm_nt(_ex) launches for a shape on the current
 * device (the decision depends on (M, N, K, flags) and the CU count only) -- the parity tests assert it so that
 * every tile variant is pinned at the shapes the training step issues.  tnr_gemm_set_option: process-wide A/B
 * switches for tools/ ("ver", "gm", "fine_pct", "allow_fine", "bm", "mix"; "pp" / "tnpp" = 0: never the queue-fed persistent
 * kernels of the NT GEMM / the weight gradient, which then take the 256x128 or 128x128 kernels; "cus" = n: plan and size the
 * persistent GEMM grids for n compute units instead of the device's, 0 = the device's - same results, pinned by
 * test_gemm_grids_sized_for_fewer_cus_bit_exact); the library never reads the environment and the defaults are the shipped
 * configuration. */
#define TNR_ROUTE_128x128 128    /* 128x128 tile, 4 waves, 2 workgroups per CU */
#define TNR_ROUTE_256x128 2128   /* 256x128 tile, 8 waves (N % 256 != 0, or option "pp" = 0) */
#define TNR_ROUTE_256x256 256    /* 256x256 tile, 8 waves, persistent (tile queue) */
#define TNR_ROUTE_224x256 224    /* 224-row variant of the same kernel (fewer wasted rows per round) */
int tnr_gemm_nt_route(int64_t M, int64_t N, int64_t K, int flags);
int tnr_gemm_set_option(const char* key, int value);
/* The row tiling of the persistent 256-column kernel on a device with n_cu compute units (host arithmetic only, no device
 * needed): *panels row panels, *tall of them 32 * *mi rows high and the others 32 rows shorter, spread evenly - panel p starts
 * at row (32 * mi - 32) * p + 32 * floor(p * tall / panels).  Chosen so that panels * N / 256 tiles fill whole rounds of the
 * workgroups (option "mix" = 0: one height).  Results do not depend on the tiling (a row's K order is the same). */
int tnr_gemm_nt_plan(int64_t M, int64_t N, int flags, int n_cu, int* mi, int* panels, int* tall);
/* The persistent GEMM kernels (tnr_gemm_nt* on the TNR_ROUTE_256x256 / 224x256 routes, and the weight gradient's for N and K
 * multiples of 256) hand out their tiles through nine 32-bit counters per (device, stream) pair, kept in a 128-entry table
 * inside the library (a __device__ array; 288 KB).  A pair is bound at its first launch (its counters are zeroed by a
 * hipMemsetAsync on that stream) and every completed launch returns them to zero, so launches need no workspace argument.
 * The table is never drained and the current device is never changed: the 129th distinct pair is refused with
 * TNR_EUNSUPPORTED (run fewer streams, or tnr_gemm_set_option("pp", 0) and ("tnpp", 0) for the kernels without a tile
 * queue).  tnr_gemm_queue_reset zeroes the calling stream's counters again (stream-ordered): only needed after a launch on
 * that stream was aborted (a device fault survived by the process), never in normal operation.
 * (Test hooks such as the CU hog live in libtnr_testhooks.so, built beside this library for tests/ and tools/ only.) */
int tnr_gemm_queue_reset(void* stream);
/* Measurement hook (bench.py's `box` object; no reference counterpart - the reference never reports a clock): while `buf` is
 * non-NULL, workgroup b < n_pairs of every persistent NT launch (TNR_ROUTE_256x256 / 224x256) writes, as it leaves, the shader
 * cycles (s_memtime) and the 100 MHz ticks (s_memrealtime) of its life to buf[2 b], buf[2 b + 1] (uint64, device memory owned
 * by the caller, 8-byte aligned): cycles / ticks x 100 = the MHz the chip held UNDER that launch.  Process-wide like the
 * options; NULL or n_pairs = 0 turns it off (the default; two scalar loads per workgroup when on).  Results unchanged. */
int tnr_gemm_clock_stamps(void* buf, int64_t n_pairs);

/* dW[N,K] (fp32) = dY[M,N]^T . X[M,K] : weight gradient of a Linear.  Reduction over M is split into
 * `splits` slabs in `ws` (fp32, splits*N*K elements) and summed in fixed order (deterministic).
 * Rows [M, Mpad) of dY and X must be zero, Mpad = roundup(M, 64) ; N % 128 == 0, K % 128 == 0.  Rows at and behind Mpad are never
 * read, nor are gap columns (lddy > N, ldx > K); gap columns of dW (lddw > K) keep their contents.  `splits` is clamped to the number
 * of 64-row tiles and then to the number of non-empty splits: slabs of `ws` past that count are not touched.
 * accumulate != 0 adds into dW.  _ex: dW (+)= out_scale * dY^T X (the fp16 build's backward runs on loss-scaled
 * gradients; 1 / scale is applied here so that parameter gradients are the true ones, run.py:194). */
int tnr_gemm_tn_wgrad(const void* dY, int64_t lddy, const void* X, int64_t ldx, float* dW, int64_t lddw,
                      int64_t M, int64_t N, int64_t K, float* ws, int splits, int accumulate, void* stream);
int tnr_gemm_tn_wgrad_ex(const void* dY, int64_t lddy, const void* X, int64_t ldx, float* dW, int64_t lddw,
                         int64_t M, int64_t N, int64_t K, float* ws, int splits, int accumulate, float out_scale,
                         void* stream);
int64_t tnr_gemm_tn_ws_elems(int64_t N, int64_t K, int splits);
/* Up to four weight gradients - the Linears of one encoder layer that share a backward step (modeling.py:287, 305-306 and the
 * q / k / v + output Linears of :205-231) - in ONE persistent launch + one slab-sum launch: the (split, tile) units of all of
 * them are pulled from one queue, each computed exactly as in its own tnr_gemm_tn_wgrad_ex call (same unit partition, same slab
 * order: bit-identical results).  Every problem has its own `ws`.  Problems off the 256 x 256 route (N or K not a multiple of
 * 256) make the call fall back to one launch per problem.
 * accumulate == 2 CHAINS a problem to its predecessor: another row range of the same gradient (same dW, N, K, lddw, out_scale;
 * operands and M of its own) - the two encoder passes of a stage-1 step, Post-train_KD.ipynb cell 12, whose autograd sums their
 * contributions to every shared weight.  Its `ws` is ignored: its slabs follow the predecessor's in the chain HEAD's workspace,
 * which must hold (sum of the chain's `splits`) * N * K floats, and ONE fixed-order slab sum covers the chain (the head's
 * `accumulate` decides whether dW is overwritten or added to). */
typedef struct {
    const void* dY; int64_t lddy;
    const void* X; int64_t ldx;
    float* dW; int64_t lddw;
    int64_t M, N, K;
    float* ws;               /* splits * N * K fp32, this problem's own (chained problems: see above) */
    int splits, accumulate;
    float out_scale;
} tnr_wgrad_problem_t;
int tnr_gemm_tn_wgrad_group(const tnr_wgrad_problem_t* problems, int n, void* stream);

/* LayerNorm over the last dim (H = 256, 512, 768 or 1024), eps inside the sqrt (torch.nn.LayerNorm).
 * fwd: y = LN(x) ; stats (M,2) fp32 = (mean, rstd) kept for backward, or NULL: y alone, the same bits.
 * Forward and backward read only rows [0, M) of x, dy and stats and write only rows [0, M) of y, dx and dxm. */
int tnr_ln_fwd(const void* x, const float* gamma, const float* beta, float eps, void* y, float* stats,
               int64_t M, int H, void* stream);
/* bwd: dx = LN'(dy) ; partial sums go to part (nblk,3,H) fp32 then are reduced into dgamma, dbeta and
 * dxsum = column sums of dx (the bias gradient of the Linear in front of this LayerNorm); each may be null.
 * With all three null and part given, only the partials (exactly nblk = tnr_ln_bwd_blocks(M) rows of [dgamma|dbeta|dxsum]:
 * 32 rows of x per partial row below M = 32768, 128 from there on) are written and the caller reduces them
 * (tnr_reduce_multi); the rest of the workspace is left alone.
 * The call forms: all three sums ; dgamma and dbeta adjacent (dbeta == dgamma + H: one reduction for both) ; all three null
 * with part ; any one of the three alone ; part null (then all three must be null): dx only.  dx is the same bits in every form.
 * When a sum is requested, part is scratch: the reduction may overwrite it.  dxsum sums the ROUNDED 16-bit dx. */
int tnr_ln_bwd(const void* dy, const void* x, const float* stats, const float* gamma, void* dx,
               float* dgamma, float* dbeta, float* dxsum, float* part, int64_t M, int H, void* stream);
int64_t tnr_ln_bwd_part_elems(int64_t M, int H);   /* workspace good for every row count <= M */
int64_t tnr_ln_bwd_blocks(int64_t M);              /* partial rows (nblk) written for exactly M rows */

/* BertSelfAttention.multi_head_attention (tnlrv3/modeling.py:205-231) for L <= 32, head size 64:
 * softmax(Q K^T / 8 + mask_add + rel) V, heads merged.  qkv (N*L, 3*A*64) bf16 = [q | k | v];
 * rel (A,32,32) fp32 from tnr_relpos_table ; ctx (N*L, A*64) bf16.
 * mask_add (N,32) fp32 as tnr_embed_ln_fwd writes it.  Precondition: |q.k| / 8 + |rel| < 4400 for every (query, key) - the range
 * in which the reference's -10000 masks at all.  Under it a key j with mask_add[n][j] - max_k mask_add[n][k] <= -9000 has
 * probability exactly 0.0f, and the forward and backward kernels do not read its K and V rows (they may hold anything, NaN
 * included); relative to the row's maximum, so a sequence whose keys are all padding (-10000 everywhere) keeps every key. */
int tnr_attn_l32_fwd(const void* qkv, const float* mask_add, const float* rel, void* ctx,
                     int64_t n_seq, int L, int A, void* stream);
/* backward: recomputes the probabilities ; dqkv (N*L, 3*A*64) bf16 ; bias_part (N, 3*A*64) fp32 (nullable) =
 * per-sequence column sums of dqkv (rows sum to the q/k/v bias gradient). */
int tnr_attn_l32_bwd(const void* qkv, const float* mask_add, const float* rel, const void* dctx,
                     void* dqkv, float* bias_part, int64_t n_seq, int L, int A, void* stream);

/* The same attention for longer sequences (L <= 512: stage-1 title/body matching, Post-train_KD.ipynb cell 4-14):
 * flash-style 32-key tiles with an online softmax.  mask_add (N, Lr), rel (A, Lr, Lr) from tnr_embed_ln_fwd /
 * tnr_relpos_table with Lr = roundup(L, 32); lse (N, A, Lr) fp32 out (kept for backward).  As for the l32 pair, qkv, ctx, dctx
 * and dqkv must be 16-byte aligned (16-byte vector loads and stores): TNR_EINVAL otherwise. */
int tnr_attn_long_fwd(const void* qkv, const float* mask_add, const float* rel, void* ctx, float* lse,
                      int64_t n_seq, int L, int A, void* stream);
/* backward in two deterministic passes (dQ per query tile, dK/dV per key tile); delta (N, A, Lr) fp32 workspace */
int tnr_attn_long_bwd(const void* qkv, const float* mask_add, const float* rel, const void* ctx, const void* dctx,
                      const float* lse, float* delta, void* dqkv, int64_t n_seq, int L, int A, void* stream);

/* column sums (bias gradients): out[n] (+)= sum_m X[m,n] ; X bf16 or fp32 (dtype) ; part (nblk,N) fp32 scratch.
 * N % 4 == 0, ldx % 4 == 0, ldx >= N.  Only [0, M) x [0, N) of X is read: never a gap column (N .. ldx), a row behind M
 * or, batched, the space between two matrices. */
int tnr_colsum(const void* X, int64_t ldx, int dtype, int64_t M, int64_t N, float* out, float* part,
               int accumulate, void* stream);
/* batch of matrices X + z*sX -> out (batch, N) ; part needs batch * tnr_colsum_part_elems(M, N) */
int tnr_colsum_batched(const void* X, int64_t ldx, int64_t sX, int dtype, int64_t M, int64_t N, int batch,
                       float* out, float* part, int accumulate, void* stream);
int64_t tnr_colsum_part_elems(int64_t M, int64_t N);

/* ---- heads ----------------------------------------------------------------------------------- */

/* AttentionPooling over the L tokens of each title, no mask (model_bert.py:15-34 called at :133).
 * e (N*L, lde) fp32 = tanh(fc1 y) from tnr_gemm_nt ; w2 (Q) ; b2 scalar.  Forward and backward, in both forms, read only the
 * columns q < Q of e (the GEMM that writes e leaves zeros in its padded columns; these kernels do not depend on it).
 * out: nv (N,H) fp32, alpha (N,Lr) fp32 normalised weights (Lr = roundup(L,32), L <= 512), den (N) fp32 = sum exp + 1e-8. */
int tnr_attpool_fwd(const void* y, const float* e, int64_t lde, const float* w2, const float* b2, int Q,
                    float* nv, float* alpha, float* den, int64_t n_seq, int L, int H, void* stream);
/* backward: dnv (N,H) fp32 -> dy_direct (N*L,H) bf16 = alpha*dnv ; dpre (N*L, lddpre) bf16 =
 * d tanh-preactivation (padded cols 0) ; dw2_part (N,Q) ; db2_part (N) ; db1_part (N, lddpre) nullable = per-title
 * column sums of dpre (fc1 bias gradient partials). */
int tnr_attpool_bwd(const void* y, const float* e, int64_t lde, const float* w2, int Q, const float* dnv,
                    const float* alpha, const float* den, void* dy_direct, void* dpre, int64_t lddpre,
                    float* dw2_part, float* db2_part, float* db1_part, int64_t n_seq, int L, int H, void* stream);

/* The same pooling (model_bert.py:15-34) for FEW, LONG sequences - the bodies of stage 1 (Post-train_KD.ipynb cell 12: 32 x 512
 * tokens): token-parallel parts run per (sequence, 64-token chunk) or one wave per token instead of one workgroup per sequence;
 * same arguments and outputs plus a caller-owned workspace of tnr_attpool_long_ws_elems(n_seq, L, H, Q, lddpre) floats.  Outputs
 * equal tnr_attpool_fwd / _bwd up to fp32 rounding (chunk partials are combined in chunk order: deterministic). */
int64_t tnr_attpool_long_ws_elems(int64_t n_seq, int L, int H, int Q, int64_t lddpre);
int tnr_attpool_fwd_long(const void* y, const float* e, int64_t lde, const float* w2, const float* b2, int Q,
                         float* nv, float* alpha, float* den, float* ws, int64_t n_seq, int L, int H, void* stream);
int tnr_attpool_bwd_long(const void* y, const float* e, int64_t lde, const float* w2, int Q, const float* dnv,
                         const float* alpha, void* dy_direct, void* dpre, int64_t lddpre, float* dw2_part,
                         float* db2_part, float* db1_part, float* ws, int64_t n_seq, int L, int H, void* stream);

/* NewsEncoder pooling 'cls' (mean = 0: hidden state of token 0) or mean over all L positions (mean = 1), model_bert.py:
 * 130-135: y (n_seq*L, H) 16-bit -> nv (n_seq, H) fp32 ; backward dnv -> dy (every row written). */
int tnr_pool_fwd(const void* y, float* nv, int64_t n_seq, int L, int H, int mean, void* stream);
int tnr_pool_bwd(const float* dnv, void* dy, int64_t n_seq, int L, int H, int mean, void* stream);

/* small fp32 GEMM on the f32 MFMA (exact fp32):  for z in [0,batch):
 *   C_z[m,n] = alpha * sum_k A_z(m,k) B_z(n,k) + bias_z[n] + beta * C_z[m,n]
 * A_z(m,k) = A[z*sA + m*a_rs + k*a_cs] (a_idx must be NULL), likewise B.  ksplit > 1 splits K over workgroups
 * into part (ksplit, batch, M, N) fp32 (caller's workspace) and a second kernel sums the slices in fixed order and
 * applies alpha / bias / beta: the fp32 MFMA issues one 32x32x2 block per 64 cycles, so a workgroup's time is
 * K * 32 cycles whatever the tile count -- few-tile GEMMs with a long K are latency-sized unless K is split. */
int tnr_sgemm(const float* A, int64_t a_rs, int64_t a_cs, int64_t sA, const int32_t* a_idx,
              const float* B, int64_t b_rs, int64_t b_cs, int64_t sB,
              float* C, int64_t ldc, int64_t sC, const float* bias, int64_t sBias,
              int64_t M, int64_t N, int64_t K, int batch, float alpha, float beta,
              int ksplit, float* part, void* stream);

/* Up to 8 independent tnr_sgemm problems in ONE launch (+ one launch that reduces every split problem): the heads' GEMMs are
 * latency-sized, so problems that do not depend on each other cost the longest of them instead of their sum.  Each problem is
 * computed exactly as tnr_sgemm computes it (same tiles, same K split rule, same summation order): identical bits.  The
 * problem array is HOST memory, read at the call. */
typedef struct tnr_sgemm_problem {
    const float* A; int64_t a_rs, a_cs, sA;
    const float* B; int64_t b_rs, b_cs, sB;
    float* C; int64_t ldc, sC;
    const float* bias; int64_t sBias;
    int64_t M, N, K;
    int batch;
    float alpha, beta;
    int ksplit;
    float* part;             /* ksplit > 1: (ksplit, batch, M, N) fp32 workspace of THIS problem (not shared inside a group) */
} tnr_sgemm_problem_t;
int tnr_sgemm_group(const tnr_sgemm_problem_t* problems, int n, void* stream);

/* out = [a (na) | b (nb)]: the step's news indices as one array - history slots (B*U) then candidate slots (B*C), the row
 * order of the encoder pass (dataloader.py:129-138 at index level; replaces a torch.cat inside the step) */
int tnr_concat_i32(const int32_t* a, int64_t na, const int32_t* b, int64_t nb, int32_t* out, void* stream);

/* out[z, out_row0 + r, :] = tbl[z, idx[r], :]  (dataloader.py:140-144 teacher-embedding gather, done on
 * device from resident tables instead of on the host) */
int tnr_gather_rows(const float* tbl, int64_t R, const int32_t* idx, int64_t n_idx, int D, int n_model,
                    float* out, int64_t out_rows, int64_t out_row0, void* stream);

/* In-batch de-duplication of news (SURVEY.md appendix iii: identical input rows encode to the same vector): the
 * encoder runs once per distinct news id of the step, tnr_gather_rows expands the vectors to the (B*U + B*C) slots
 * (dataloader.py:131,138 at index level) and this entry point folds the slot gradients back:
 *   out[u,:] = sum_{j in [seg[u], seg[u+1])} src[order[j],:]      (fixed order, no atomics)
 * order (n_slots) = slot ids grouped by distinct id, seg (n_seg+1) offsets; empty segments give zero rows. */
int tnr_segment_sum_rows(const float* src, const int32_t* order, const int32_t* seg, int64_t n_seg, int D,
                         float* out, void* stream);

/* Deterministic row scatter-sum (the backward of an embedding lookup, tnlrv3/modeling.py:138, 153-178): for every run of equal
 * keys in keys_sorted (n, ascending),   table[key, :] (+)= sum over the run of src[order[j], :]   in increasing j with a fixed
 * reduction tree (tnr_segment_sum_rows' scheme); the runs are found on the device.  order (n) = row of src per sorted position
 * (the permutation a stable sort of the keys returns), every entry in [0, rows of src).  Keys equal to skip_key (padding_idx: that
 * row never gets a gradient) and keys outside [0, table_rows) are skipped; rows no key names are NOT touched (the caller zeroes
 * the table region).  No floating-point atomics: bit-identical from run to run.  D % 4 == 0, D <= 2048. */
int tnr_scatter_sum_rows(const float* src, int64_t n, int D, const int32_t* keys_sorted, const int32_t* order, int32_t skip_key,
                         float* table, int64_t table_rows, int accumulate, void* stream);

/* UserEncoder.forward (model_bert.py:155-176, model != NRMS) + scorer bmm (:204 / :286-287) for
 * `n_model` encoders at once (student and/or frozen teachers), one workgroup per (impression, model).
 * vec: (n_model, R, D) fp32 row tables ; hidx (B,U) / cidx (B,C) int32 row ids ; mask (B,U) fp32.
 * params are stacked per model: pad (n_model,D), w1 (n_model,Q,D), b1 (n_model,Q), w2 (n_model,Q), b2 (n_model).
 * epre (n_model, B*U, Q) = fc1 pre-activations v W1^T + b1 of every history slot in position order (one batched
 * tnr_sgemm) ; epad (n_model, Q) = fc1(pad_doc) of every model, or NULL to have each workgroup compute it ;
 * epre == NULL: fc1 runs INSIDE the kernel on the fp32 MFMA (one launch per pass; needs D % 8 == 0 and
 * 64 (D + 4) + U Q + D + 64 floats of LDS), epad is ignored ;
 * out: user (model z at user + z*user_stride, (B,D)), score (n_model,B,C), saved e (n_model,B,U,Q), alpha (n_model,B,U), den (n_model,B). */
int tnr_user_score_fwd(const float* vec, int64_t R, const int32_t* hidx, const int32_t* cidx, const float* mask,
                       const float* pad, const float* w1, const float* b1, const float* w2, const float* b2,
                       int user_log_mask, const float* epre, const float* epad, float* user, int64_t user_stride, float* score,
                       float* e, float* alpha, float* den, int n_model, int B, int U, int C, int D, int Q, void* stream);
/* backward of the student's user encoder (model_bert.py:155-176), in two kernels around two fp32 GEMMs the caller
 * issues with tnr_sgemm:
 *   tnr_user_bwd_pre : hv (B*U, D) = blended history rows in position order ; dpre (B*U, Q) = gradient of the fc1
 *                      pre-activation ; part (B, 2Q + D + 1) = per-impression partials [b1 | w2 | pad | b2]
 *   caller           : dW1 (Q,D) = dpre^T hv ;  dhv (B*U, D) = dpre W1
 *   tnr_user_bwd_post: dvec[hidx[b,u]] += (alpha * duser + dhv) * m ; fills the pad_doc partial of `part`.
 * Rows of dvec (the contract of tnr_user_bwd_post, tnr_user_blend_bwd and tnr_score_bwd alike): one workgroup per impression
 * adds into dvec with plain loads and stores, so the rows named by DIFFERENT impressions must be distinct - a row shared by two
 * impressions is a race.  A row named more than once WITHIN one impression is fine: each thread walks its impression's slots
 * serially, the repeats are summed in slot order.  Callers whose impressions share rows (in-batch de-duplication) pass slot
 * indices (hidx / cidx = arange over the slots of a gathered table) and fold the slot gradients with tnr_segment_sum_rows
 * afterwards, as tiny-newsrec_amd/engine.py does. */
int tnr_user_bwd_pre(const float* vec, const int32_t* hidx, const float* mask, const float* pad, const float* w2,
                     int user_log_mask, const float* duser, const float* e, const float* alpha, float* hv,
                     float* dpre, float* part, int B, int U, int D, int Q, void* stream);
int tnr_user_bwd_post(const float* dhv, const float* alpha, const float* duser, const float* mask,
                      const int32_t* hidx, int user_log_mask, float* dvec, float* part, int B, int U, int D, int Q,
                      void* stream);
int64_t tnr_user_bwd_part_stride(int D, int Q);
/* NRMS user encoder (args.model == 'NRMS': model_bert.py:37-100, 145-148, 162-164, 171-173), d_k = d_v = 16, for
 * `n_model` encoders at once (student and/or frozen teachers); fp32.
 *   tnr_user_blend_fwd : hv (n_model, B*U, D) = vec[hidx] * m + pad * (1-m) (user_log_mask 0) | vec[hidx] (1)
 *   caller             : qkv (n_model, B*U, 3*Dh) = hv [W_Q;W_K;W_V]^T + b   (tnr_sgemm), Dh = n_heads*16
 *   tnr_nrms_attn_fwd  : ctx (n_model, B*U, Dh) ; sc = exp(q.k/4) [* mask_j if use_mask] / (sum + 1e-8), raw exp (:51-58)
 *   tnr_nrms_attn_bwd  : dctx (B*U, Dh) -> dqkv (B*U, 3*Dh) for one model, recomputing sc (two fixed-order phases)
 *   tnr_user_blend_bwd : dvec[hidx] += dhv * m ; pad_part[b*part_stride + d] = sum_u dhv * (1-m)
 *                        (rows of different impressions distinct, repeats within one summed in slot order: see tnr_user_bwd_post) */
int tnr_user_blend_fwd(const float* vec, int64_t R, const int32_t* hidx, const float* mask, const float* pad,
                       int user_log_mask, float* hv, int n_model, int B, int U, int D, void* stream);
int tnr_user_blend_bwd(const float* dhv, const float* mask, const int32_t* hidx, int user_log_mask, float* dvec,
                       float* pad_part, int64_t part_stride, int B, int U, int D, void* stream);
int tnr_nrms_attn_fwd(const float* qkv, const float* mask, int use_mask, float* ctx, int64_t ctx_rows, int n_model,
                      int B, int U, int n_heads, void* stream);   /* ctx rows of model z start at z*ctx_rows (>= B*U) */
int tnr_nrms_attn_bwd(const float* qkv, const float* mask, int use_mask, const float* dctx, float* dqkv, int B,
                      int U, int n_heads, void* stream);

/* backward of the scorer bmm (model_bert.py:204): dvec[cidx[b,c]] += dscore[b,c]*user[b] ;
 * duser[b] += sum_c dscore[b,c]*vec[cidx[b,c]].  Rows cidx names in different impressions must be distinct, repeats within one
 * impression are summed in slot order (see tnr_user_bwd_post); callers with shared rows gather to slots first and fold with
 * tnr_segment_sum_rows. */
int tnr_score_bwd(const float* vec, const int32_t* cidx, const float* user, const float* dscore, float* dvec,
                  float* duser, int B, int C, int D, void* stream);

/* Model.forward losses (model_bert.py:271, 288-305; kd_ce_loss :208-219): teacher CE -> weights
 * softmax(-CE) -> mixed soft labels -> distill + coef*target, and d/d student_score.
 * s_score (B,C) ; t_score (T,B,C) ; out: tw (B,T), dscore (B,C), losses[0..1] = distill, target. */
int tnr_kd_score_loss(const float* s_score, const float* t_score, const int64_t* label, float temperature,
                      float coef, float* tw, float* dscore, float* losses, int B, int C, int T, void* stream);
/* embedding KD (model_bert.py:277-284, 300-303) on stacked rows [B*U history | B*C candidate | B user]:
 * S (Rtot,D) student rows ; P (T,Rtot,D) projected teacher rows ; tw (B,T) ; Rtot = B*(U+C+1).
 * U = 0 is the stage-1 layout [B*C titles | B bodies] (Post-train_KD.ipynb cell 14).
 * out: emb loss (scalar) ; dS (Rtot,D) ; dP (T,Rtot,D) ; part (Rtot) workspace. */
int tnr_kd_embed_loss(const float* S, const float* P, const float* tw, float* loss, float* dS, float* dP,
                      float* part, int B, int U, int C, int D, int T, void* stream);

/* out[i] (+)= sum_r part[r*stride + i] , i < n  (fixed order).  `part` is scratch: tall inputs are first summed
 * in place per row chunk, so its contents are clobbered. */
int tnr_reduce_rows(const float* part, int64_t rows, int64_t stride, int64_t n, float* out, int accumulate,
                    void* stream);

/* many fixed-order row reductions in ONE launch: desc = n_blocks x 6 int64 on the device, one per workgroup,
 * {src ptr, rows, row stride in floats, ncols <= 64, dst ptr, accumulate | (fp32 bits of scale) << 32}:
 * dst[c] (+)= scale * sum_r src[r*stride + c] ; upper half 0 = scale 1.
 * Callers reduce tall partial matrices in two launches (row chunks in place, then the chunk rows). */
int tnr_reduce_multi(const int64_t* desc, int n_blocks, void* stream);
/* x[i] *= s , i < n (fp32) */
int tnr_scale_inplace(float* x, int64_t n, float s, void* stream);

/* ---- dropout (train-mode) variants: the same operations with a dropout site, see tnr_dropout_t ------------------
 * The two embedding variants (mask after the LayerNorm, tnlrv3/modeling.py:177) also take pos_ids: NULL = position i of token i
 * (BERT / UniLM), else an int32 table laid out like the token table (n_seq or n+1 rows x L) naming each token's position row --
 * RoBERTa's cumulative non-pad count + padding_idx (PLM-NR --model_type roberta, PLM-NR/utils.py:17-21). */
int tnr_embed_ln_fwd_do(const int64_t* tok, int64_t n_seq, int L, int H, const float* word, const float* pos,
                        const float* type0, const float* gamma, const float* beta, float eps, void* out, float* mask_add,
                        const tnr_dropout_t* drop, const int32_t* pos_ids, void* stream);
int tnr_embed_ln_fwd_indexed_do(const int32_t* news_combined, const int32_t* nidx, int64_t n_seq, int L, int H,
                                const float* word, const float* pos, const float* type0, const float* gamma,
                                const float* beta, float eps, void* out, float* mask_add, const tnr_dropout_t* drop,
                                const int32_t* pos_ids, void* stream);
/* C = epilogue(A . B^T) with the site's mask on (acc + bias [-> activation]) BEFORE the residual add:
 * BertSelfOutput / BertOutput = dense -> dropout -> LayerNorm(x + residual).  Mask element index = m * N + n. */
int tnr_gemm_nt_do(const void* A, int64_t lda, const void* B, int64_t ldb, void* C, int64_t ldc,
                   int64_t M, int64_t N, int64_t K, const float* bias, const void* res, int64_t ldres,
                   void* aux, int64_t ldaux, int flags, float* colsum_part, const tnr_dropout_t* drop, void* stream);
/* LayerNorm backward behind such a Linear: dx (the residual branch's gradient) and dxm = dx * mask / (1 - p) (the Linear's
 * output gradient: what its weight gradient, dgrad and bias gradient consume; the dxsum partials are sums of dxm). */
int tnr_ln_bwd_do(const void* dy, const void* x, const float* stats, const float* gamma, void* dx,
                  float* dgamma, float* dbeta, float* dxsum, float* part, int64_t M, int H, void* dxm,
                  const tnr_dropout_t* drop, void* stream);
/* The same two with a row-major site split at a row (stage 1's joint passes: the body pass's token rows laid directly behind
 * the title pass's, one launch over both): rows [0, split_row) under `drop`, rows [split_row, M) under `drop_tail` (same seed,
 * site and p, its own call) with the row index counted from split_row - exactly the masks of the two per-pass _do calls.
 * drop_tail NULL or split_row == M: bit-identical to the _do call.  TNR_EINVAL if the sites differ in seed, site or p, or if
 * split_row is outside [0, M]. */
int tnr_gemm_nt_do_split(const void* A, int64_t lda, const void* B, int64_t ldb, void* C, int64_t ldc,
                         int64_t M, int64_t N, int64_t K, const float* bias, const void* res, int64_t ldres,
                         void* aux, int64_t ldaux, int flags, float* colsum_part, const tnr_dropout_t* drop,
                         const tnr_dropout_t* drop_tail, int64_t split_row, void* stream);
int tnr_ln_bwd_do_split(const void* dy, const void* x, const float* stats, const float* gamma, void* dx,
                        float* dgamma, float* dbeta, float* dxsum, float* part, int64_t M, int H, void* dxm,
                        const tnr_dropout_t* drop, const tnr_dropout_t* drop_tail, int64_t split_row, void* stream);
/* attention with dropout on the normalised probabilities (:224); backward regenerates the mask */
int tnr_attn_l32_fwd_do(const void* qkv, const float* mask_add, const float* rel, void* ctx, int64_t n_seq, int L, int A,
                        const tnr_dropout_t* drop, void* stream);
int tnr_attn_l32_bwd_do(const void* qkv, const float* mask_add, const float* rel, const void* dctx, void* dqkv,
                        float* bias_part, int64_t n_seq, int L, int A, const tnr_dropout_t* drop, void* stream);
int tnr_attn_long_fwd_do(const void* qkv, const float* mask_add, const float* rel, void* ctx, float* lse, int64_t n_seq,
                         int L, int A, const tnr_dropout_t* drop, void* stream);
int tnr_attn_long_bwd_do(const void* qkv, const float* mask_add, const float* rel, const void* ctx, const void* dctx,
                         const float* lse, float* delta, void* dqkv, int64_t n_seq, int L, int A,
                         const tnr_dropout_t* drop, void* stream);
/* the multipliers (0 or 1 / (1 - p)) of a site as fp32, for tests: row-major (rows, cols) sites, and the attention
 * probabilities (pairs = n_seq * A, L, L) through the per-query (by_columns = 0) or per-key (1) device accessor */
int tnr_dropout_mask(const tnr_dropout_t* drop, int64_t rows, int64_t cols, float* out, void* stream);
int tnr_dropout_mask_probs(const tnr_dropout_t* drop, int64_t pairs, int L, int by_columns, float* out, void* stream);
/* tnr_dropout_mask of a site split at a row (the rule of the *_do_split entry points) */
int tnr_dropout_mask_split(const tnr_dropout_t* drop, const tnr_dropout_t* drop_tail, int64_t split_row, int64_t rows, int64_t cols,
                           float* out, void* stream);

/* ---- optimiser ------------------------------------------------------------------------------- */

/* torch.optim.Adam(amsgrad=True) (run.py:134) on a flat fp32 parameter buffer ; step = 1-based count.
 * grad_scale multiplies g first (1/world for the data-parallel average, run.py:145-149).
 * vmax == NULL: plain Adam (Post-train_KD.ipynb cell 18). */
int tnr_amsgrad_step(float* p, const float* g, float* m, float* v, float* vmax, int64_t n, int step,
                     float lr, float beta1, float beta2, float eps, float grad_scale, void* stream);

/* Dynamic loss scaling of the fp16 build (the reference trains in fp32 and needs none, run.py:134,194-195; with 16-bit
 * activation gradients one overflow would otherwise poison m / v / vmax for good).  guard = 4 uint32 words on the device,
 * zero at start: [0] stamp of the last step that overflowed, [1] number of skipped steps, [2], [3] unused.
 * tnr_grad_nonfinite: if any of g[0 .. n) is inf or nan, guard[0] = max(guard[0], stamp) and guard[1] += 1 (stamp >= 1, the
 * caller's running count of optimiser steps; two launches: the scan, in which only a workgroup that found something touches
 * guard, and a one-thread kernel that counts the skip).  tnr_amsgrad_step_guarded = tnr_amsgrad_step, except that (a) a launch whose
 * stamp equals guard[0] touches nothing: the skipped step; (b) Adam's bias corrections use step - (guard[1] - known_skips):
 * `step` is the caller's count of steps, known_skips how many skipped ones it has already taken out of that count (it learns of
 * a skip with a lag of up to two steps).  Stream-ordered, no host synchronisation; the caller reads guard back whenever it
 * likes (tiny-newsrec_amd/engine.py: LossScaler).  guard == NULL: unguarded. */
int tnr_grad_nonfinite(const float* g, int64_t n, unsigned* guard, unsigned stamp, void* stream);
/* the same in pieces, for a gradient that arrives bucket by bucket (data parallelism: each bucket is scanned as soon as its
 * all-reduce has landed, beside the collectives still in flight): any number of _scan launches over disjoint slices with one
 * stamp (they only ever raise guard[0] to it), then ONE _commit that counts the skipped step.  scan(all) + commit ==
 * tnr_grad_nonfinite. */
int tnr_grad_nonfinite_scan(const float* g, int64_t n, unsigned* guard, unsigned stamp, void* stream);
int tnr_grad_nonfinite_commit(unsigned* guard, unsigned stamp, void* stream);
int tnr_amsgrad_step_guarded(float* p, const float* g, float* m, float* v, float* vmax, int64_t n, int step,
                             float lr, float beta1, float beta2, float eps, float grad_scale, const unsigned* guard,
                             unsigned stamp, unsigned known_skips, void* stream);

/* Gradient clipping by global norm: torch.nn.utils.clip_grad_norm_(parameters, max_norm, norm_type = 2) on the gradient the
 * optimiser consumes, grad_scale * g (the reference has none; an extension, engine.py: Engine.step(max_grad_norm=...)).  State on
 * the device: part = tnr_grad_sumsq_parts(n) floats per scanned slice, laid one slice behind the other by the caller, and clip =
 * 2 floats, [0] the coefficient min(1, max_norm / (norm + 1e-6)), [1] norm = grad_scale * sqrt(sum g^2).
 * tnr_grad_sumsq_scan: ONE pass over the 16-byte-aligned slice g[0 .. n) writes part[0 .. tnr_grad_sumsq_parts(n)), one fp32 sum
 * of squares per workgroup, and - guard != NULL - raises guard[0] to stamp exactly as tnr_grad_nonfinite_scan does for the same
 * data (the fp16 build reads its gradient once for both).  Fixed order: per lane four running sums (one per component of its
 * 16-byte reads, one fma per element), their pairwise sum, the 64 lanes of a wave by butterfly, the four waves in wave order,
 * one plain store; no float atomics and no arrival counter, the only atomic is the guard's fetch_max from an offending
 * workgroup.  The grid depends on n alone (tnr_grad_sumsq_parts: host-only, no GPU needed), so the bits are a function of
 * (n, values).
 * tnr_grad_clip_commit: one workgroup sums part[0 .. n_part) in double in a fixed order and stores clip[0], clip[1]; a sum of
 * squares that overflowed fp32 gives norm = inf and coefficient 0, a NaN gives NaN, as torch's fp32 computation does.
 * tnr_amsgrad_step_clipped = tnr_amsgrad_step_guarded with grad_scale * clip[0] in place of grad_scale (guard == NULL stays
 * legal: bf16).  All stream-ordered, no host synchronisation; the caller reads clip back whenever it likes. */
int64_t tnr_grad_sumsq_parts(int64_t n);
int tnr_grad_sumsq_scan(const float* g, int64_t n, float* part, unsigned* guard, unsigned stamp, void* stream);
int tnr_grad_clip_commit(const float* part, int64_t n_part, float max_norm, float grad_scale, float* clip, void* stream);
int tnr_amsgrad_step_clipped(float* p, const float* g, float* m, float* v, float* vmax, int64_t n, int step,
                             float lr, float beta1, float beta2, float eps, float grad_scale, const unsigned* guard,
                             unsigned stamp, unsigned known_skips, const float* clip, void* stream);

/* Gradient accumulation over micro-batches (the reference has none; an extension, engine.py: Engine.backward(micro=(j, K))).  One
 * streaming pass over two fp32 buffers laid out alike (the flat gradient and an accumulator, or slices of them):
 *   overwrite != 0:  dst[i] = src[i] for i in [0, n).  dst is NOT READ: whatever it held (an inf / nan of an abandoned window
 *                    included) is gone, and the pass moves 8 bytes per element;
 *   overwrite == 0:  dst[i] = dst[i] + src[i]: ONE IEEE fp32 add per element - no scale, no fma, nothing reassociated - so the
 *                    bits are a function of the two inputs alone; 12 bytes per element.
 * inf and nan propagate as IEEE addition propagates them (inf + -inf = nan), which is how an fp16 overflow in ANY micro-batch
 * reaches the gradient the overflow guard scans.  The three uses: the first micro-batch (acc <- g), the ones between (acc += g)
 * and the last (g += acc, dst the gradient buffer or one bucket's slice of it).  dst and src non-NULL, 16-byte aligned and
 * different, n >= 1; anything else returns TNR_EINVAL and launches nothing.  Stream-ordered, no host synchronisation. */
int tnr_grad_accum(float* dst, const float* src, int64_t n, int overwrite, void* stream);

/* Decoupled weight decay and a learning-rate schedule in the fused update: torch.optim.AdamW(amsgrad = vmax != NULL) with
 * lr_scheduler.LambdaLR semantics (the reference has neither; an extension, engine.py: Engine.step(weight_decay=, warmup_steps=,
 * lr_decay_steps=)).  tnr_adamw_step = tnr_amsgrad_step_guarded / _clipped (guard and clip both nullable) with
 *   - THREE learning rates: lr_k is the (scheduled) rate of the update if t_k = max(step - k, 1) updates have been taken, this one
 *     included, k = 0, 1, 2 - the candidates the bias corrections already have, picked on the device by guard[1] - known_skips
 *     (k >= 2 -> lr2), so a schedule follows the updates TAKEN and a skipped step advances neither Adam's count nor the schedule.
 *     The caller computes them (engine.lr_schedule: linear warmup from 0, then linear decay or constant); lr0 == lr1 == lr2 and
 *     weight_decay == 0 give the bits of tnr_amsgrad_step / _guarded / _clipped.
 *   - weight_decay >= 0, decoupled, in torch's order: for an element whose bit is set in decay_bits, p <- p * (1 - lr_k *
 *     weight_decay) first, then the Adam / AMSGrad update on the UNDECAYED gradient grad_scale * g (x clip[0] when clip is given:
 *     the decay does not see the clip coefficient).  lr_k * weight_decay is formed on the host in double.  A launch stamped
 *     guard[0] decays nothing.
 *   - decay_bits: one bit per element of the WHOLE flat buffer the slice p[0 .. n) was cut from, uint32 words on the device,
 *     element e = bit (e & 31) of word e >> 5; `first` = the slice's element offset in that buffer, a multiple of 4 (as the
 *     16-byte alignment of p implies when the buffer is 16-byte aligned), so a thread's four bits never straddle a word.  The map
 *     must hold at least (first + n + 31) / 32 words.  NULL is legal iff weight_decay == 0; then the map and `first` are not read
 *     and the kernel is the one without decay.
 * Errors (no launch): first % 4 != 0 or < 0, weight_decay > 0 with a NULL map, weight_decay < 0, and everything
 * tnr_amsgrad_step_guarded refuses. */
int tnr_adamw_step(float* p, const float* g, float* m, float* v, float* vmax, int64_t n, int step, float lr0, float lr1,
                   float lr2, float beta1, float beta2, float eps, float grad_scale, float weight_decay,
                   const unsigned* decay_bits, int64_t first, const unsigned* guard, unsigned stamp, unsigned known_skips,
                   const float* clip, void* stream);

/* An exponential moving average of the parameters inside the fused update: torch.optim.swa_utils.AveragedModel with
 * get_ema_multi_avg_fn(decay) / TF's ExponentialMovingAverage (the reference has none; an extension, engine.py:
 * Engine.step(ema_decay=, ema_warmup=)).  tnr_adamw_step_ema = tnr_adamw_step (guard, clip and decay_bits nullable under the same
 * rules; lr0 == lr1 == lr2 with weight_decay == 0 is plain Adam / AMSGrad with an average) with
 *   - ema: fp32, 16-byte aligned, laid out like p - the SAME slice of the average's buffer as p[0 .. n) is of the parameters'.
 *     Once an element's new parameter p_new is formed (still in registers), ema <- ema + w_k (p_new - ema), one fma: +4 bytes
 *     read and +4 written per element on the update's 36 (AMSGrad) or 28 (Adam).  p, m, v, vmax get the bits tnr_adamw_step gives.
 *   - THREE weights w_k = 1 - decay_k in [0, 1], k = 0, 1, 2: the weight of this update if t_k = max(step - k, 1) updates have
 *     been taken, this one included - picked on the device by guard[1] - known_skips together with lr_k and the bias corrections
 *     (k >= 2 -> w2), so a warm-up of the decay (engine.ema_decay_at) follows the updates TAKEN.  The caller forms them in double
 *     and rounds once.  w = 0 leaves the average's bits; w = 1 gives p_new up to the rounding of the difference.
 *   - A launch stamped guard[0] (the skipped step) returns before touching ema: a skipped step does not advance the average.
 * Errors (no launch): ema == NULL or not 16-byte aligned, a w_k outside [0, 1] or NaN, and everything tnr_adamw_step refuses. */
int tnr_adamw_step_ema(float* p, const float* g, float* m, float* v, float* vmax, int64_t n, int step, float lr0, float lr1,
                       float lr2, float beta1, float beta2, float eps, float grad_scale, float weight_decay,
                       const unsigned* decay_bits, int64_t first, const unsigned* guard, unsigned stamp, unsigned known_skips,
                       const float* clip, float* ema, float w0, float w1, float w2, void* stream);

/* LAMB (You et al., "Large Batch Optimization for Deep Learning", Algorithm 2): per-tensor trust ratios on the Adam / AMSGrad
 * moments (the reference has none; an extension, engine.py: Engine.step(lamb=True)).  Per trainable tensor w, with g = grad_scale
 * (x clip[0] when clip is given) x the flat gradient, exactly what tnr_adamw_step consumes:
 *   1. m = b1 m + (1 - b1) g, v = b2 v + (1 - b2) g^2; vmax != NULL (AMSGrad): vhat = max(vmax, v), stored; else vhat = v.
 *   2. r = (m / c1) / (sqrt(vhat) / sqrt(c2) + eps), c1 = 1 - b1^t, c2 = 1 - b2^t: the bias corrections of tnr_amsgrad_step.
 *   3. u = r + weight_decay * w on the elements of a tensor of the decay set, u = r elsewhere.  The decay is COUPLED (it is part
 *      of the update the trust ratio scales), not AdamW's p *= 1 - lr wd.
 *   4. A tensor of the decay set is ADAPTED, whatever weight_decay is: trust = ||w||_2 / ||u||_2, or 1 if either norm is 0 (a
 *      zero tensor can leave zero, a zero update divides nothing).  Every other tensor: trust = 1, the plain Adam update.  No
 *      clamp, no phi; a NaN or infinite norm propagates into trust.
 *   5. w <- w - lr_k * trust * u, then (ema != NULL) ema <- ema + w_k (w_new - ema) as tnr_adamw_step_ema does.
 * The element-to-tensor map is a CHUNK TABLE made by the caller (engine.py: lamb_chunks): n_chunks entries of four int32 {first
 * element, count in 1 .. 4096, tensor id, flags (bit 0: the tensor is in the decay set)}; a chunk never crosses its tensor's end,
 * the chunks of a tensor are consecutive in the table, and what no chunk covers (alignment gaps, reserved rows) is neither read
 * nor written.  `first` is an offset into p / g / m / v / vmax / ema, which are the WHOLE flat buffers (16-byte aligned, n
 * elements, n < 2^31); a chunk may start at any element: 16-byte accesses where the absolute address allows, scalars at the
 * unaligned head and tail.  The table is passed twice, on the device (16-byte aligned) and as the host's copy of the same entries,
 * which is what the entry point checks before it launches.  The tensor table (tnr_lamb_commit) has n_tensors entries of four
 * int32 {first chunk, number of chunks, adapted (0 / 1), 0}, on the device and on the host likewise.
 *   tnr_lamb_norms: one workgroup per chunk forms m, v, vhat and u in registers, STORES NONE OF THEM, and writes part[2 j] = the
 *     sum of w^2 and part[2 j + 1] = the sum of u^2 of the launch's j-th chunk if its flag is set (the partials of other chunks
 *     are not written).  Fixed order: per lane four running sums (one per component of its 16-byte reads, scalars into the
 *     first), their pairwise sum, the 64 lanes by butterfly, the four waves in wave order, one plain store.
 *   tnr_lamb_commit: per tensor, the partials of its chunks summed in double in a fixed order -> trust[t], and for diagnostics
 *     trust[n_tensors + t] = ||w||, trust[2 n_tensors + t] = ||u|| (3 n_tensors floats; not adapted: 1, 0, 0).
 *   tnr_lamb_step: the same chunks (any consecutive part of the table, so that ranges with different rates get a launch each):
 *     recomputes m, v, vhat, u by the same expressions - the same bits as in the norm pass -, stores the moments, updates w with
 *     trust[tensor], then the average.  lr_k, w_k: the three candidates of tnr_adamw_step_ema.
 * Guard (nullable) and candidates as in tnr_amsgrad_step_guarded: each of the three launches, stamped guard[0], returns before
 * touching p, m, v, vmax, ema, part and trust; otherwise the bias corrections, the rate and the average's weight are those of
 * candidate min(guard[1] - known_skips, 2), the SAME one in the norm pass and the apply pass (u depends on c1 and c2).  No float
 * atomics and no arrival counters: the bits of trust and of every buffer are a function of the inputs alone.
 * Errors (no launch): a NULL or misaligned buffer or table, n_chunks < 1, n_tensors < 1, a chunk outside [0, n) or with a count
 * outside 1 .. 4096 or a tensor id >= n_tensors, a tensor whose chunks lie outside [0, n_chunks), step < 1, weight_decay < 0, a
 * guard with stamp 0, and for tnr_lamb_step with an average a weight outside [0, 1].  Stream-ordered, no host synchronisation. */
int tnr_lamb_norms(const float* p, const float* g, const float* m, const float* v, const float* vmax, int64_t n,
                   const int32_t* chunks, const int32_t* chunks_host, int64_t n_chunks, int n_tensors, int step, float beta1,
                   float beta2, float eps, float grad_scale, float weight_decay, const unsigned* guard, unsigned stamp,
                   unsigned known_skips, const float* clip, float* part, void* stream);
int tnr_lamb_commit(const float* part, int64_t n_chunks, const int32_t* tensors, const int32_t* tensors_host, int n_tensors,
                    float* trust, const unsigned* guard, unsigned stamp, void* stream);
int tnr_lamb_step(float* p, const float* g, float* m, float* v, float* vmax, int64_t n, const int32_t* chunks,
                  const int32_t* chunks_host, int64_t n_chunks, int n_tensors, int step, float lr0, float lr1, float lr2,
                  float beta1, float beta2, float eps, float grad_scale, float weight_decay, const unsigned* guard, unsigned stamp,
                  unsigned known_skips, const float* clip, const float* trust, float* ema, float w0, float w1, float w2,
                  void* stream);

/* refresh bf16 weight copies after an update: desc = n_desc * 8 int64 on DEVICE:
 * {src fp32 ptr, rows, cols, dst ptr (or 0), dst ld, dstT ptr (or 0), dstT ld, unused}
 * dst[r*ld + c] = bf16(src[r,c]) ; dstT[c*ldT + r] = bf16(src[r,c]), round to nearest even.  Only [0, rows) x [0, cols) of
 * each copy is written (ld >= cols, ldT >= rows: the gap columns keep what they held). */
int tnr_refresh_shadows(const int64_t* desc, int n_desc, int64_t total_tiles, const int64_t* tile_start,
                        void* stream);

/* elementwise helpers */
int tnr_cast_f32_to_bf16(const float* src, void* dst, int64_t n, void* stream);
int tnr_cast_bf16_to_f32(const void* src, float* dst, int64_t n, void* stream);

/* ---- fp16 activations ------------------------------------------------------------------------------
 * Every entry point that touches 16-bit tensors exists a second time with the suffix _f16: identical
 * signature and semantics with IEEE half instead of bf16 (same MFMA rate, 3 more mantissa bits: the build used
 * for the 1e-3 parity bound).  The sources that touch the 16-bit type are compiled twice (-DTNR_BUILD_F16). */
int tnr_embed_ln_fwd_f16(const int64_t* tok, int64_t n_seq, int L, int H, const float* word, const float* pos,
                     const float* type0, const float* gamma, const float* beta, float eps,
                     void* out, float* mask_add, void* stream);
int tnr_embed_ln_fwd_indexed_f16(const int32_t* news_combined, const int32_t* nidx, int64_t n_seq, int L, int H,
                             const float* word, const float* pos, const float* type0, const float* gamma,
                             const float* beta, float eps, void* out, float* mask_add, void* stream);
int tnr_embed_ln_bwd_f16(const int64_t* tok, int64_t n_seq, int L, int H, const void* dy, const float* word, const float* pos,
                     const float* type0, const float* gamma, float eps, float inv_scale, float* dx, float* part,
                     const tnr_dropout_t* drop, const int32_t* pos_ids, void* stream);
int tnr_embed_ln_bwd_indexed_f16(const int32_t* news_combined, const int32_t* nidx, int64_t n_seq, int L, int H, const void* dy,
                             const float* word, const float* pos, const float* type0, const float* gamma, float eps,
                             float inv_scale, float* dx, float* part, const tnr_dropout_t* drop, const int32_t* pos_ids,
                             void* stream);
int tnr_gemm_nt_f16(const void* A, int64_t lda, const void* B, int64_t ldb, void* C, int64_t ldc,
                int64_t M, int64_t N, int64_t K, const float* bias, const void* res, int64_t ldres,
                void* aux, int64_t ldaux, int flags, void* stream);
int tnr_gemm_nt_ex_f16(const void* A, int64_t lda, const void* B, int64_t ldb, void* C, int64_t ldc,
                   int64_t M, int64_t N, int64_t K, const float* bias, const void* res, int64_t ldres,
                   void* aux, int64_t ldaux, int flags, float* colsum_part, void* stream);
int64_t tnr_gemm_colsum_rows_f16(int64_t M);
int tnr_gemm_nt_route_f16(int64_t M, int64_t N, int64_t K, int flags);
int tnr_gemm_tn_wgrad_f16(const void* dY, int64_t lddy, const void* X, int64_t ldx, float* dW, int64_t lddw,
                      int64_t M, int64_t N, int64_t K, float* ws, int splits, int accumulate, void* stream);
int tnr_gemm_tn_wgrad_ex_f16(const void* dY, int64_t lddy, const void* X, int64_t ldx, float* dW, int64_t lddw,
                         int64_t M, int64_t N, int64_t K, float* ws, int splits, int accumulate, float out_scale,
                         void* stream);
int64_t tnr_gemm_tn_ws_elems_f16(int64_t N, int64_t K, int splits);
int tnr_gemm_tn_wgrad_group_f16(const tnr_wgrad_problem_t* problems, int n, void* stream);
int tnr_ln_fwd_f16(const void* x, const float* gamma, const float* beta, float eps, void* y, float* stats,
               int64_t M, int H, void* stream);
int tnr_ln_bwd_f16(const void* dy, const void* x, const float* stats, const float* gamma, void* dx,
               float* dgamma, float* dbeta, float* dxsum, float* part, int64_t M, int H, void* stream);
int tnr_pool_fwd_f16(const void* y, float* nv, int64_t n_seq, int L, int H, int mean, void* stream);
int tnr_pool_bwd_f16(const float* dnv, void* dy, int64_t n_seq, int L, int H, int mean, void* stream);
int tnr_attn_long_fwd_f16(const void* qkv, const float* mask_add, const float* rel, void* ctx, float* lse,
                          int64_t n_seq, int L, int A, void* stream);
int tnr_attn_long_bwd_f16(const void* qkv, const float* mask_add, const float* rel, const void* ctx, const void* dctx,
                          const float* lse, float* delta, void* dqkv, int64_t n_seq, int L, int A, void* stream);
int tnr_attn_l32_fwd_f16(const void* qkv, const float* mask_add, const float* rel, void* ctx,
                     int64_t n_seq, int L, int A, void* stream);
int tnr_attn_l32_bwd_f16(const void* qkv, const float* mask_add, const float* rel, const void* dctx,
                     void* dqkv, float* bias_part, int64_t n_seq, int L, int A, void* stream);
int tnr_colsum_f16(const void* X, int64_t ldx, int dtype, int64_t M, int64_t N, float* out, float* part,
               int accumulate, void* stream);
int tnr_colsum_batched_f16(const void* X, int64_t ldx, int64_t sX, int dtype, int64_t M, int64_t N, int batch,
                       float* out, float* part, int accumulate, void* stream);
int tnr_attpool_fwd_f16(const void* y, const float* e, int64_t lde, const float* w2, const float* b2, int Q,
                    float* nv, float* alpha, float* den, int64_t n_seq, int L, int H, void* stream);
int tnr_attpool_bwd_f16(const void* y, const float* e, int64_t lde, const float* w2, int Q, const float* dnv,
                    const float* alpha, const float* den, void* dy_direct, void* dpre, int64_t lddpre,
                    float* dw2_part, float* db2_part, float* db1_part, int64_t n_seq, int L, int H, void* stream);
int64_t tnr_attpool_long_ws_elems_f16(int64_t n_seq, int L, int H, int Q, int64_t lddpre);
int tnr_attpool_fwd_long_f16(const void* y, const float* e, int64_t lde, const float* w2, const float* b2, int Q,
                         float* nv, float* alpha, float* den, float* ws, int64_t n_seq, int L, int H, void* stream);
int tnr_attpool_bwd_long_f16(const void* y, const float* e, int64_t lde, const float* w2, int Q, const float* dnv,
                         const float* alpha, void* dy_direct, void* dpre, int64_t lddpre, float* dw2_part,
                         float* db2_part, float* db1_part, float* ws, int64_t n_seq, int L, int H, void* stream);
int tnr_refresh_shadows_f16(const int64_t* desc, int n_desc, int64_t total_tiles, const int64_t* tile_start,
                        void* stream);
int tnr_cast_f32_to_bf16_f16(const float* src, void* dst, int64_t n, void* stream);
int tnr_cast_bf16_to_f32_f16(const void* src, float* dst, int64_t n, void* stream);

int tnr_embed_ln_fwd_do_f16(const int64_t* tok, int64_t n_seq, int L, int H, const float* word, const float* pos,
                        const float* type0, const float* gamma, const float* beta, float eps, void* out, float* mask_add,
                        const tnr_dropout_t* drop, const int32_t* pos_ids, void* stream);
int tnr_embed_ln_fwd_indexed_do_f16(const int32_t* news_combined, const int32_t* nidx, int64_t n_seq, int L, int H,
                                const float* word, const float* pos, const float* type0, const float* gamma,
                                const float* beta, float eps, void* out, float* mask_add, const tnr_dropout_t* drop,
                                const int32_t* pos_ids, void* stream);
int tnr_gemm_nt_do_f16(const void* A, int64_t lda, const void* B, int64_t ldb, void* C, int64_t ldc,
                   int64_t M, int64_t N, int64_t K, const float* bias, const void* res, int64_t ldres,
                   void* aux, int64_t ldaux, int flags, float* colsum_part, const tnr_dropout_t* drop, void* stream);
int tnr_ln_bwd_do_f16(const void* dy, const void* x, const float* stats, const float* gamma, void* dx,
                  float* dgamma, float* dbeta, float* dxsum, float* part, int64_t M, int H, void* dxm,
                  const tnr_dropout_t* drop, void* stream);
int tnr_gemm_nt_do_split_f16(const void* A, int64_t lda, const void* B, int64_t ldb, void* C, int64_t ldc,
                             int64_t M, int64_t N, int64_t K, const float* bias, const void* res, int64_t ldres,
                             void* aux, int64_t ldaux, int flags, float* colsum_part, const tnr_dropout_t* drop,
                             const tnr_dropout_t* drop_tail, int64_t split_row, void* stream);
int tnr_ln_bwd_do_split_f16(const void* dy, const void* x, const float* stats, const float* gamma, void* dx,
                            float* dgamma, float* dbeta, float* dxsum, float* part, int64_t M, int H, void* dxm,
                            const tnr_dropout_t* drop, const tnr_dropout_t* drop_tail, int64_t split_row, void* stream);
int tnr_attn_l32_fwd_do_f16(const void* qkv, const float* mask_add, const float* rel, void* ctx, int64_t n_seq, int L, int A,
                        const tnr_dropout_t* drop, void* stream);
int tnr_attn_l32_bwd_do_f16(const void* qkv, const float* mask_add, const float* rel, const void* dctx, void* dqkv,
                        float* bias_part, int64_t n_seq, int L, int A, const tnr_dropout_t* drop, void* stream);
int tnr_attn_long_fwd_do_f16(const void* qkv, const float* mask_add, const float* rel, void* ctx, float* lse, int64_t n_seq,
                         int L, int A, const tnr_dropout_t* drop, void* stream);
int tnr_attn_long_bwd_do_f16(const void* qkv, const float* mask_add, const float* rel, const void* ctx, const void* dctx,
                         const float* lse, float* delta, void* dqkv, int64_t n_seq, int L, int A,
                         const tnr_dropout_t* drop, void* stream);

/* ---------------------------------------------------------------------------------------------------------------------------
 * Top-K retrieval (csrc/retrieve.hip): of all Nn news, the K each user should see.  The reference stops at per-impression dot
 * products on the host (Tiny-NewsRec/run.py:254-262); this is the serving step the student exists for.
 *   s(u, n) = sum_k users[u, k] * news[n, k], an fp32 fma chain on the exact fp32 MFMA whose k order depends on D alone: a
 *   (user row, news row) pair has the same score bits in every call, tile, split and launch position.
 * Row n is eligible for user u when first_row <= n < Nn, n is not among excl[u, 0:E] (excl may be NULL with E = 0; entries outside
 * [first_row, Nn) are ignored, duplicates allowed) and s(u, n) is not NaN.  a is before b iff s_a > s_b, or s_a == s_b and
 * n_a < n_b.  Row u of out_idx / out_score (each (Nu, K), dense) is the first K eligible rows in that order with the kernel's own
 * score bits; slots beyond the eligible rows hold idx -1, score -inf.
 * The news range is cut into `splits` contiguous parts (0 = the library chooses from Nu, Nn and the CU count; never more parts
 * than 8192 / K, 1024, or tiles of 128 rows): one workgroup per (user tile, part) writes a partial list into `work`, a second
 * launch merges them (skipped for one part).  The outputs are bit-identical for every `splits`.  No float atomics.
 * Limits: 1 <= K <= 128, D % 4 == 0, 4 <= D <= 1024, E <= 512, Nn < 2^31, strides >= D / >= E (16-byte aligned operands with
 * strides % 4 == 0 take 16-byte loads, others scalar ones).  Anything else, a null pointer or work_bytes below
 * tnr_topk_workspace launches nothing and returns TNR_EINVAL.  tnr_topk_workspace: bytes, host arithmetic only (no device
 * is asked: it plans splits = 0 for 256 CUs); 0 for a bad request. */
int64_t tnr_topk_workspace(int64_t Nu, int64_t Nn, int K, int splits);
int tnr_topk_scores(const float* users, int64_t u_rs, int64_t Nu, const float* news, int64_t n_rs, int64_t Nn, int64_t first_row,
                    int D, const int32_t* excl, int64_t e_rs, int E, int K, int32_t* out_idx, float* out_score, int splits,
                    void* work, int64_t work_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------------------------------------
 * Rank metrics of the eval path (csrc/evaluate.hip): what the reference computes per impression on the host
 * (Tiny-NewsRec/run.py:254-262: one dot product per candidate, then roc_auc_score, mrr_score, ndcg_score at 5 and 10).
 * Impressions are ragged: impression b owns cand / label / scores [offs[b], offs[b + 1]) (offs int32 (B + 1), non-decreasing from
 * 0); cand holds rows of `news` in [0, Nn) - row 0, the padding news, is scored like any other - and label 0 or 1.  A candidate
 * outside [0, Nn) is never read and scores NaN.
 *   Score: s(u, n) = the fp32 fma chain over k = 0, 1, ..., D - 1 from +0 of users[u, k] * news[n, k] - tnr_topk_scores' bits for
 *   the same pair; they depend on (user row, news row, D) alone, not on the impression, its place in the launch, the strides or
 *   the width of the loads (16-byte aligned operands with strides % 4 == 0 take 16-byte loads, others scalar ones).
 *   An impression with P positives and Q = C - P negatives is skipped when P = 0 or Q = 0 (C = 0 included).
 *   Position of a positive i: r_i = #{j : s_j > s_i} + #{j > i : s_j == s_i} (float compares: among equal scores the later index
 *   ranks first, +0 == -0).  In double:
 *     AUC    = sum over positives of (#negatives s_j < s_i + 0.5 #negatives s_j == s_i) / (P Q)
 *     MRR    = (sum over positives of 1 / (r_i + 1)) / P
 *     nDCG@k = (sum over positives with r_i < k of 1 / log2(r_i + 2)) / (sum over t < min(P, k) of 1 / log2(t + 2))
 * scores (offs[B] floats, required) receives every candidate's score and is read back by the rank phase, so an impression may
 * have any number of candidates.  per (B, 4) doubles or NULL: AUC, MRR, nDCG@5, nDCG@10 of each impression, zeros where it is
 * skipped; an impression's values do not depend on its place in the launch.  acc[6] = {impressions seen, impressions scored,
 * sum AUC, sum MRR, sum nDCG@5, sum nDCG@10}: accumulate = 0 overwrites it, 1 adds this launch's totals.  The totals are summed
 * in a fixed order in double by one workgroup - no float atomics, bit-identical from run to run.  Without `per` that workgroup
 * also has to compute every impression's values again from `scores` (same bits, one CU's speed): pass `per` where time matters.
 * No allocation, no host synchronisation.  B = 0 launches the totals alone (accumulate = 0 zeroes acc) and needs only acc.
 * Limits: 1 <= D <= 1024, strides >= D, B and Nn below 2^31, acc and per 8-byte aligned.  Anything else or a null required
 * pointer launches nothing, writes nothing and returns TNR_EINVAL. */
int tnr_rank_metrics(const float* users, int64_t u_rs, int64_t B, const float* news, int64_t n_rs, int64_t Nn, int D,
                     const int32_t* offs, const int32_t* cand, const int32_t* label, float* scores, double* per, double* acc,
                     int accumulate, void* stream);

/* ---------------------------------------------------------------------------------------------------------------------------
 * In-batch negatives of the target loss (csrc/inbatch.hip; no counterpart in the reference, whose target term is a softmax over
 * an impression's own C = 1 + npratio candidates).  A batch of B impressions has M = B * C candidate slots; slot j = b' * C + c'
 * holds news id cand_ids[b', c'].  Foreign slot j is a negative of impression b - bit E[b, j] - iff
 *   1. b' != b;   2. its id is not 0 (the padding news);   3. no earlier slot j' < j holds the same id (a distinct news counts
 *   once per batch, at its first slot: this bit depends on j alone);   4. its id is not among cand_ids[b, :] (so never b's own
 *   positive);   5. its id is not among hist_ids[b, :] (all U entries, whatever the history mask says).
 * target_b = -log softmax(score[b, 0:C] U {z[b, j] : E[b, j]})[label_b] at temperature 1, z[b, j] = the fp32 fma chain over
 * k = 0, 1, ..., D - 1 from +0 of users[b, k] * cands[j, k]: tnr_topk_scores' and tnr_rank_metrics' bits for the same pair, which
 * depend on (user row, candidate row, D) alone.  E = 0 everywhere (B = 1, say) is the plain target loss.
 * tnr_inbatch_plan: ids int32 (B, U) / (B, C) -> elig (B, W) uint32 words, W = ceil(M / 32), bit j of row b = E[b, j], bits at and
 *   above M zero; count[b] int32 = the bits set in row b; first_ws: W words of workspace (rule 3's bit per slot).  Two launches.
 * tnr_inbatch_loss: users (B rows, stride u_rs), cands (M rows, stride c_rs), score (B, C), label int64 (B).  ADDS
 *   coef * (p - onehot) / B into dscore[b, :], writes the whole row dz[b, :] = coef * p_j / B (0 where E = 0) of dz (B, M), z[b, j]
 *   for eligible j only (z (B, M) or NULL), per[b] = target_b, and losses[1] = mean_b target_b (summed in a fixed order by a
 *   second, one-workgroup launch); the other losses are not touched.  The row of a slot with E[b, j] = 0 is not read for b.
 *   The sum of exponentials runs in a fixed order by RANK among the impression's eligible slots (own candidates first), and its
 *   log is taken as log1p(sum - 1): bit-identical from run to run, an impression's values do not depend on its place in the
 *   batch, and a loss of 1e-6 (a dominating positive) keeps its digits.  Limits: C <= 16, B * C <= 8192, D <= 1024, D % 4 == 0, strides >= D (16-byte aligned operands with strides % 4
 *   == 0 take 16-byte loads, others scalar ones).
 * tnr_inbatch_bwd: one launch; duser (B, D) [b] += sum over set bits j ascending of dz[b, j] cands[j], dcand (M, D) [j] += sum over
 *   b ascending with bit j set of dz[b, j] users[b].  Every row has one owner; a row without a set bit is not touched.
 * No float atomics, no allocation, no host synchronisation.  Anything outside the limits or a null required pointer launches
 * nothing, writes nothing and returns TNR_EINVAL with the limit named in tnr_last_error(). */
int tnr_inbatch_plan(const int32_t* hist_ids, const int32_t* cand_ids, uint32_t* elig, int32_t* count, uint32_t* first_ws, int B,
                     int U, int C, void* stream);
int tnr_inbatch_loss(const float* users, int64_t u_rs, const float* cands, int64_t c_rs, const float* score, const int64_t* label,
                     const uint32_t* elig, float coef, float* dscore, float* dz, float* z, float* per, float* losses, int B, int C,
                     int D, void* stream);
int tnr_inbatch_bwd(const float* dz, const uint32_t* elig, const float* users, int64_t u_rs, const float* cands, int64_t c_rs,
                    float* duser, float* dcand, int B, int C, int D, void* stream);

/* ---------------------------------------------------------------------------------------------------------------------------
 * Collectives of the data-parallel step.  Replace hvd.init / hvd.broadcast_parameters /
 * hvd.broadcast_optimizer_state (Tiny-NewsRec/run.py:141-144, utils.py:43-60) and the gradient all-reduce inside
 * hvd.DistributedOptimizer (run.py:145-149: average of the trainable parameters' gradients, fp32, no compression).
 * One process per GPU; the communicator lives on the caller's CURRENT device (the library never calls hipSetDevice); every
 * collective is asynchronous on `stream` and in place; RCCL is bound at run time (dlopen librccl.so.1: inside a PyTorch-ROCm
 * process the copy torch has loaded) - without it these return TNR_EUNSUPPORTED and nothing else in the library is affected.
 * tnr_comm_unique_id: rank 0 fills 128 bytes that reach the other ranks out of band (the host side uses the rendezvous store
 * torch.distributed already has, dist.py).  tnr_comm_allreduce_avg: average = 1 divides by the world size inside the reduction
 * (ncclAvg), 0 sums (the engine folds 1 / world into tnr_amsgrad_step's grad_scale).  tnr_comm_reduce_scatter_allgather: the same
 * result by direct exchange on the fully connected xGMI mesh (n a multiple of the world size, `shard` n / world floats of the
 * caller's).  Errors: RCCL's own code and text in tnr_last_error(), status TNR_ELAUNCH. */
typedef struct tnr_comm tnr_comm_t;
int tnr_comm_unique_id(void* id128);
int tnr_comm_init(const void* id128, int world, int rank, tnr_comm_t** comm);
int tnr_comm_world(const tnr_comm_t* comm, int* world, int* rank);
int tnr_comm_broadcast(tnr_comm_t* comm, float* buf, int64_t n, int root, void* stream);
int tnr_comm_allreduce_avg(tnr_comm_t* comm, float* buf, int64_t n, int average, void* stream);
int tnr_comm_reduce_scatter_allgather(tnr_comm_t* comm, float* buf, float* shard, int64_t n, int average, void* stream);
int tnr_comm_destroy(tnr_comm_t* comm);

#ifdef __cplusplus
}
#endif
#endif
