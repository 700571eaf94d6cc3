// Top-K news retrieval (tnr_topk_scores): every user against the whole news table, scores on the exact fp32 MFMA, selection fused
// behind the K loop so that the Nu x Nn score matrix never exists.  fp32 only: built once (ONCE in the Makefile).
//
// Phase 1 (topk_part_kernel): one workgroup per (user tile, news part).  A wave owns 32 users (the MFMA's column = its lane),
// the workgroup's NW waves share each 128-row news tile through LDS; a lane ends a tile with 64 scores of ONE user in its
// accumulators.  A score is an fma chain over k = 0, 1, 2, ... from +0 (zero padding behind D changes no bit), so its bits depend
// on (user row, news row, D) alone - not on the tile, the part or the user's place in the launch.
// Selection by threshold: a lane compares its scores with its user's current K-th best (one VALU compare per score); only when
// some lane of the wave has a survivor is the slow path entered, where ONE lane per user (the two lane halves take turns) checks
// the exact order, then the exclusion list (a 64-bit hash mask per user says when it has to be read at all), and replaces the
// user's worst kept entry: an unsorted K-entry list in LDS, j-major so that the 32 users' scans are conflict-free, in groups of
// 16 whose minima are kept beside it, so that finding the new worst reads 16 + K / 16 entries.  The lists are rank-sorted once,
// at the end.
// Entries are 64-bit keys: (order-preserving score bits) << 32 | ~index, so "before" in the contract's order is "key greater";
// key 0 is the empty slot (index -1).  -0 is stored as +0, so that the keys order +0 == -0 as the float compare does.
// Phase 2 (topk_merge_kernel): one wave per user merges the parts' sorted lists (staged in LDS) head by head.
#include "common.h"

namespace {

constexpr int TK_NT = 128;                 // news rows per tile
constexpr int TK_KC = 32;                  // k values per staged chunk
constexpr int TK_LD = TK_KC + 1;           // padded LDS row (conflict-free b32 reads of 32 rows at one k)
constexpr int TK_STAGE_BYTES = 2 * TK_NT * TK_LD * 4;
constexpr int TK_MAX_K = 128, TK_MAX_D = 1024, TK_MAX_E = 512;
constexpr int TK_GBYTES = (TK_MAX_K / 16) * 32 * 12;   // per wave: the 16-entry groups' minima (key + slot) of 32 users
constexpr int TK_LDS_MAX = 160 * 1024;
constexpr int TK_MERGE_KEYS = 8192;        // keys one merge workgroup stages (64 KB): splits * K never exceeds it
constexpr int TK_MAX_SPLITS = 1024;

typedef unsigned long long u64;

struct TopkArgs {
    const float* users; int64_t u_rs; int64_t Nu;
    const float* news; int64_t n_rs; int64_t Nn; int64_t first_row;
    int D;
    const int32_t* excl; int64_t e_rs; int E;
    int K;
    int32_t* out_idx; float* out_score;
    u64* work;                             // (Nu, S, K) keys, S > 1 only
    int S; int64_t chunk;                  // parts and rows per part
    int vec;                               // both operands allow 16-byte loads
};

__device__ __forceinline__ unsigned tk_order(float s) {
    const unsigned b = __float_as_uint(s + 0.0f);                   // -0 (a product that underflows below zero) counts and reads as +0
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float tk_unorder(unsigned o) {
    return __uint_as_float((o & 0x80000000u) ? (o ^ 0x80000000u) : ~o);
}
__device__ __forceinline__ u64 tk_key(float s, int n) { return ((u64)tk_order(s) << 32) | (unsigned)~n; }
__device__ __forceinline__ void tk_emit(u64 key, int32_t* idx, float* score) {
    if (key == 0ull) { *idx = -1; *score = -INFINITY; }
    else { *idx = (int32_t)~(unsigned)key; *score = tk_unorder((unsigned)(key >> 32)); }
}
__device__ __forceinline__ u64 tk_shfl(u64 v, int src) {
    const unsigned lo = (unsigned)__shfl((int)(unsigned)v, src, 64), hi = (unsigned)__shfl((int)(unsigned)(v >> 32), src, 64);
    return ((u64)hi << 32) | lo;
}
__device__ __forceinline__ f32x4 tk_load4(const float* p, bool vec) {
    if (vec) return *(const f32x4*)p;
    f32x4 v;
    v[0] = p[0]; v[1] = p[1]; v[2] = p[2]; v[3] = p[3];
    return v;
}

template <int NW>
__global__ __launch_bounds__(NW * 64) void topk_part_kernel(TopkArgs g) {
    constexpr int NT = NW * 64;
    constexpr int NLD = (TK_NT * (TK_KC / 4) + NT - 1) / NT;        // 16-byte pieces of a news chunk per thread
    constexpr int ULD = (NW * 32 * (TK_KC / 4)) / NT;               // of a user chunk: 4
    extern __shared__ __align__(16) unsigned char tk_smem[];
    float* Ns = (float*)tk_smem;                                     // [128][33]
    float* Us = Ns + TK_NT * TK_LD;                                  // [NW * 32][33]
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, ul = lane & 31, half = lane >> 5;
    const int K = g.K;
    u64* list = (u64*)(tk_smem + TK_STAGE_BYTES) + (size_t)w * K * 32;                           // [K][32 users] of this wave
    u64* gmin = (u64*)(tk_smem + TK_STAGE_BYTES + (size_t)NW * K * 256 + (size_t)w * TK_GBYTES);   // [8 groups][32 users]: a group's worst
    int* gpos = (int*)(gmin + (TK_MAX_K / 16) * 32);                                              // and its slot
    const int NG = (K + 15) >> 4;

    const int part = blockIdx.x % g.S;
    const int64_t u0 = (int64_t)(blockIdx.x / g.S) * (NW * 32);
    const int64_t p0 = g.first_row + (int64_t)part * g.chunk;
    const int64_t p1 = p0 + g.chunk < g.Nn ? p0 + g.chunk : g.Nn;
    const int64_t u = u0 + w * 32 + ul;
    const bool uvalid = u < g.Nu;

    for (int j = lane; j < K * 32; j += 64) list[j] = 0ull;
    // bit (n & 63) is set when some row n of this part is on the user's exclusion list: the list itself is read only for those
    u64 exmask = 0ull;
    if (uvalid)
        for (int e = half; e < g.E; e += 2) {
            const int x = g.excl[u * g.e_rs + e];
            if (x >= p0 && x < p1) exmask |= 1ull << (x & 63);
        }
    exmask |= tk_shfl(exmask, lane ^ 32);

    const int nkc = (g.D + TK_KC - 1) / TK_KC;
    const int ntiles = p1 > p0 ? (int)((p1 - p0 + TK_NT - 1) / TK_NT) : 0;
    const int nit = ntiles * nkc;

    f32x4 nv[NLD], uv[ULD];
    auto fetch = [&](int tile, int kc) {
        const int64_t n0 = p0 + (int64_t)tile * TK_NT;
        const int k0 = kc * TK_KC;
#pragma unroll
        for (int q = 0; q < NLD; ++q) {
            const int i = tid + q * NT, row = i >> 3, k = k0 + (i & 7) * 4;
            const int64_t n = n0 + row;
            const bool ok = i < TK_NT * (TK_KC / 4) && n < g.Nn && k < g.D;
            nv[q] = ok ? tk_load4(g.news + n * g.n_rs + k, g.vec) : f32x4{0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int q = 0; q < ULD; ++q) {
            const int i = tid + q * NT, row = i >> 3, k = k0 + (i & 7) * 4;
            const int64_t uu = u0 + row;
            uv[q] = (uu < g.Nu && k < g.D) ? tk_load4(g.users + uu * g.u_rs + k, g.vec) : f32x4{0.f, 0.f, 0.f, 0.f};
        }
    };

    f32x16 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

    // the user's selection state, kept equal in its two lanes: entries kept, the worst of them (valid once cnt == K)
    int cnt = 0, minpos = 0;
    u64 minkey = 0ull;
    float thr = -INFINITY;

    int tile = 0, kc = 0;
    if (nit > 0) fetch(0, 0);
    for (int it = 0; it < nit; ++it) {
#pragma unroll
        for (int q = 0; q < NLD; ++q) {
            const int i = tid + q * NT;
            if (i < TK_NT * (TK_KC / 4)) {
                float* d = Ns + (i >> 3) * TK_LD + (i & 7) * 4;
                d[0] = nv[q][0]; d[1] = nv[q][1]; d[2] = nv[q][2]; d[3] = nv[q][3];
            }
        }
#pragma unroll
        for (int q = 0; q < ULD; ++q) {
            const int i = tid + q * NT;
            float* d = Us + (i >> 3) * TK_LD + (i & 7) * 4;
            d[0] = uv[q][0]; d[1] = uv[q][1]; d[2] = uv[q][2]; d[3] = uv[q][3];
        }
        __syncthreads();
        int ntile = tile, nkcn = kc + 1;
        if (nkcn == nkc) { nkcn = 0; ++ntile; }
        if (it + 1 < nit) fetch(ntile, nkcn);                       // the next chunk's loads fly under this chunk's MFMAs
        const float* up = Us + (w * 32 + ul) * TK_LD + half;
        const float* np = Ns + ul * TK_LD + half;
#pragma unroll 4
        for (int kk = 0; kk < TK_KC; kk += 2) {                     // k ascending: the order depends on D alone
            const float b = up[kk];
#pragma unroll
            for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(np[t * 32 * TK_LD + kk], b, acc[t], 0, 0, 0);
        }
        __syncthreads();
        if (kc == nkc - 1) {
            // ---- selection: acc[t][r] = s(user of this lane, news n0 + 32 t + (r & 3) + 8 (r >> 2) + 4 half)
            const int64_t n0 = p0 + (int64_t)tile * TK_NT;
            bool anyp = false;
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) anyp |= acc[t][r] >= thr;          // false for NaN
            if (__ballot(anyp && uvalid) != 0ull) {
#pragma unroll 1
                for (int t = 0; t < 4; ++t) {
                    const f32x16 a = t == 0 ? acc[0] : t == 1 ? acc[1] : t == 2 ? acc[2] : acc[3];
#pragma unroll 1
                    for (int h = 0; h < 2; ++h) {
                        // the lane's survivors of this sub-tile as a bit mask; the wave then takes them one per lane and turn, so a
                        // turn costs one pass through the body however many lanes have one
                        unsigned m = 0u;
                        const int64_t nb = n0 + t * 32 + 4 * half;
#pragma unroll
                        for (int r = 0; r < 16; ++r)
                            m |= (half == h && uvalid && a[r] >= thr && nb + (r & 3) + 8 * (r >> 2) < p1) ? 1u << r : 0u;
                        while (__ballot(m != 0u) != 0ull) {
                            if (m != 0u) {
                                const int r = __ffs(m) - 1;
                                m &= m - 1u;
                                float sr = a[0];
#pragma unroll
                                for (int q = 1; q < 16; ++q) sr = r == q ? a[q] : sr;
                                const int n = (int)(nb + (r & 3) + 8 * (r >> 2));
                                const u64 key = tk_key(sr, n);
                                bool take = cnt < K || key > minkey;
                                if (take && ((exmask >> (n & 63)) & 1ull)) {       // only then can n be on the user's list
                                    int hit = 0;
                                    const int32_t* ex = g.excl + u * g.e_rs;
#pragma unroll 8
                                    for (int e = 0; e < g.E; ++e) hit |= ex[e] == n;
                                    take = !hit;
                                }
                                if (take) {
                                    const bool full = cnt == K;
                                    const int slot = full ? minpos : cnt;
                                    list[slot * 32 + ul] = key;
                                    cnt += full ? 0 : 1;
                                    if (cnt == K) {
                                        // the worst kept entry again: the slot's group of 16, then the groups' minima
                                        const int gfirst = full ? slot >> 4 : 0, glast = full ? slot >> 4 : NG - 1;
                                        u64 mk = ~0ull; int mp = 0;
                                        for (int gi = gfirst; gi <= glast; ++gi) {
                                            const int je = gi * 16 + 16 < K ? gi * 16 + 16 : K;
                                            mk = ~0ull;
#pragma unroll 4
                                            for (int j = gi * 16; j < je; ++j) {
                                                const u64 kj = list[j * 32 + ul];
                                                if (kj < mk) { mk = kj; mp = j; }
                                            }
                                            gmin[gi * 32 + ul] = mk;
                                            gpos[gi * 32 + ul] = mp;
                                        }
                                        if (NG > 1) {
                                            mk = ~0ull;
                                            int mg = 0;
#pragma unroll 4
                                            for (int gi = 0; gi < NG; ++gi) {
                                                const u64 kg = gmin[gi * 32 + ul];
                                                if (kg < mk) { mk = kg; mg = gi; }
                                            }
                                            mp = gpos[mg * 32 + ul];
                                        }
                                        minkey = mk; minpos = mp; thr = tk_unorder((unsigned)(mk >> 32));
                                    }
                                }
                            }
                        }
                        __builtin_amdgcn_wave_barrier();
                        const int src = ul + 32 * h;                 // the half that just ran owns the state
                        cnt = __shfl(cnt, src, 64);
                        minpos = __shfl(minpos, src, 64);
                        thr = __shfl(thr, src, 64);
                        minkey = tk_shfl(minkey, src);
                    }
                }
            }
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
        }
        tile = ntile; kc = nkcn;
    }
    __syncthreads();

    // ---- rank-sort each user's list (keys are distinct but for the empty slots, which keep their order) and write it out
    for (int x = 0; x < 32; ++x) {
        const int64_t ux = u0 + w * 32 + x;
        if (ux >= g.Nu) break;
        for (int j = lane; j < K; j += 64) {
            const u64 kj = list[j * 32 + x];
            int rank = 0;
            for (int i = 0; i < K; ++i) {
                const u64 ki = list[i * 32 + x];
                rank += (ki > kj) || (ki == kj && i < j);
            }
            if (g.S > 1) g.work[(ux * g.S + part) * K + rank] = kj;
            else tk_emit(kj, g.out_idx + ux * K + rank, g.out_score + ux * K + rank);
        }
    }
}

// one wave per user: S sorted K-lists -> the first K of their union
__global__ __launch_bounds__(64) void topk_merge_kernel(const u64* __restrict__ work, int S, int K, int32_t* __restrict__ out_idx,
                                                        float* __restrict__ out_score) {
    extern __shared__ __align__(16) unsigned char tk_smem[];
    __shared__ int ptr[TK_MAX_SPLITS];
    u64* keys = (u64*)tk_smem;                                       // [S][K]
    const int lane = threadIdx.x;
    const int64_t u = blockIdx.x;
    const u64* src = work + u * S * K;
    const int n = S * K;
    for (int i0 = 0; i0 < n; i0 += 64 * 8) {                         // eight loads in flight per lane
        u64 v[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) v[q] = i0 + q * 64 + lane < n ? src[i0 + q * 64 + lane] : 0ull;
#pragma unroll
        for (int q = 0; q < 8; ++q)
            if (i0 + q * 64 + lane < n) keys[i0 + q * 64 + lane] = v[q];
    }
    for (int p = lane; p < S; p += 64) ptr[p] = 0;
    __syncthreads();
    // part p belongs to lane p % 64 for the whole merge; a lane keeps the best head of its parts and looks again only after
    // it has given one away
    u64 best = 0ull; int bp = -1;
    auto heads = [&]() {
        best = 0ull; bp = -1;
        for (int p = lane; p < S; p += 64) {
            const int j = ptr[p];
            const u64 kj = j < K ? keys[p * K + j] : 0ull;
            if (kj > best) { best = kj; bp = p; }
        }
    };
    heads();
    for (int k = 0; k < K; ++k) {
        u64 top = best;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const u64 other = tk_shfl(top, lane ^ o);
            top = other > top ? other : top;
        }
        if (top != 0ull && best == top) {                            // real keys are distinct: exactly one lane
            ptr[bp] += 1;
            heads();
        }
        if (lane == 0) tk_emit(top, out_idx + u * K + k, out_score + u * K + k);
    }
}

int tk_waves(int64_t Nu, int K) {
    int nw = (int)((Nu + 31) / 32 < 4 ? (Nu + 31) / 32 : 4);
    while (nw > 1 && TK_STAGE_BYTES + nw * (K * 256 + TK_GBYTES) > TK_LDS_MAX) --nw;
    return nw < 1 ? 1 : nw;
}
// parts actually cut for a request (0 = choose: the kernel runs one wave per SIMD, so a CU holds 4 / waves workgroups at a time -
// as many parts as fill the chip once, measured best (EXPERIMENTS.md item 72); a part is at least one tile)
int tk_splits(int64_t Nu, int64_t Nn, int K, int splits, int n_cu) {
    int64_t s = splits;
    if (s <= 0) {
        const int nw = tk_waves(Nu, K);
        const int64_t tiles_u = (Nu + nw * 32 - 1) / (nw * 32);
        s = (int64_t)n_cu * (4 / nw) / tiles_u;
        const int64_t most = (Nn + TK_NT - 1) / TK_NT;
        if (s > most) s = most;
    }
    if (s > TK_MAX_SPLITS) s = TK_MAX_SPLITS;
    if (s > TK_MERGE_KEYS / K) s = TK_MERGE_KEYS / K;
    return s < 1 ? 1 : (int)s;
}
constexpr int TK_PLAN_CUS = 256;           // the CU count tnr_topk_workspace plans for (it never asks a device): MI355X's

}  // namespace

extern "C" int64_t tnr_topk_workspace(int64_t Nu, int64_t Nn, int K, int splits) {
    if (Nu < 1 || Nn < 0 || K < 1 || K > TK_MAX_K || splits < 0) return 0;
    const int s = tk_splits(Nu, Nn, K, splits, TK_PLAN_CUS);
    return s > 1 ? Nu * (int64_t)s * K * 8 : 0;
}

extern "C" int tnr_topk_scores(const float* users, int64_t u_rs, int64_t Nu, const float* news, int64_t n_rs, int64_t Nn,
                               int64_t first_row, int D, const int32_t* excl, int64_t e_rs, int E, int K, int32_t* out_idx,
                               float* out_score, int splits, void* work, int64_t work_bytes, void* stream) {
    TNR_CHECK_ARG(users && news && out_idx && out_score, "tnr_topk_scores: null pointer");
    TNR_CHECK_ARG(K >= 1 && K <= TK_MAX_K, "tnr_topk_scores: K = %d outside 1..%d", K, TK_MAX_K);
    TNR_CHECK_ARG(D >= 4 && D % 4 == 0 && D <= TK_MAX_D, "tnr_topk_scores: D = %d must be a multiple of 4, at most %d", D, TK_MAX_D);
    TNR_CHECK_ARG(E >= 0 && E <= TK_MAX_E && (E == 0 || excl) && (E == 0 || e_rs >= E), "tnr_topk_scores: E = %d outside 0..%d, or no list", E, TK_MAX_E);
    TNR_CHECK_ARG(Nu >= 1 && Nn >= 0 && Nn < (1ll << 31) && first_row >= 0 && u_rs >= D && n_rs >= D && splits >= 0,
                  "tnr_topk_scores: bad shape (Nu %ld, Nn %ld, first_row %ld, strides %ld / %ld, splits %d)", (long)Nu, (long)Nn,
                  (long)first_row, (long)u_rs, (long)n_rs, splits);
    const int n_cu = device_cus() < TK_PLAN_CUS ? device_cus() : TK_PLAN_CUS;
    int S = tk_splits(Nu, Nn, K, splits, n_cu);
    const int64_t need = tnr_topk_workspace(Nu, Nn, K, splits);
    TNR_CHECK_ARG(work_bytes >= need && (need == 0 || (work && ((uintptr_t)work & 7) == 0)),
                  "tnr_topk_scores: workspace of %ld bytes, tnr_topk_workspace says %ld (8-byte aligned)", (long)work_bytes, (long)need);
    const int64_t range = Nn > first_row ? Nn - first_row : 0;
    int64_t chunk = ((range + S - 1) / S + TK_NT - 1) / TK_NT * TK_NT;           // whole tiles per part
    if (chunk < TK_NT) chunk = TK_NT;
    S = range > 0 ? (int)((range + chunk - 1) / chunk) : 1;                      // never more than asked for
    const int nw = tk_waves(Nu, K);
    const int64_t tiles_u = (Nu + nw * 32 - 1) / (nw * 32);
    TNR_CHECK_ARG(tiles_u * S < (1ll << 31), "tnr_topk_scores: %ld workgroups", (long)(tiles_u * S));
    TopkArgs g{users, u_rs, Nu, news, n_rs, Nn, first_row, D, excl, e_rs, E, K, out_idx, out_score, (u64*)work, S, chunk,
               (((uintptr_t)users | (uintptr_t)news) & 15) == 0 && u_rs % 4 == 0 && n_rs % 4 == 0};
    const size_t lds = TK_STAGE_BYTES + (size_t)nw * (K * 256 + TK_GBYTES);
    TNR_ONCE_PER_DEVICE({
        (void)hipFuncSetAttribute((const void*)topk_part_kernel<1>, hipFuncAttributeMaxDynamicSharedMemorySize, TK_LDS_MAX);
        (void)hipFuncSetAttribute((const void*)topk_part_kernel<2>, hipFuncAttributeMaxDynamicSharedMemorySize, TK_LDS_MAX);
        (void)hipFuncSetAttribute((const void*)topk_part_kernel<3>, hipFuncAttributeMaxDynamicSharedMemorySize, TK_LDS_MAX);
        (void)hipFuncSetAttribute((const void*)topk_part_kernel<4>, hipFuncAttributeMaxDynamicSharedMemorySize, TK_LDS_MAX);
        (void)hipFuncSetAttribute((const void*)topk_merge_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, TK_MERGE_KEYS * 8);
    });
    const dim3 grid((unsigned)(tiles_u * S));
    hipStream_t st = (hipStream_t)stream;
    switch (nw) {
        case 1: hipLaunchKernelGGL(topk_part_kernel<1>, grid, dim3(64), lds, st, g); break;
        case 2: hipLaunchKernelGGL(topk_part_kernel<2>, grid, dim3(128), lds, st, g); break;
        case 3: hipLaunchKernelGGL(topk_part_kernel<3>, grid, dim3(192), lds, st, g); break;
        default: hipLaunchKernelGGL(topk_part_kernel<4>, grid, dim3(256), lds, st, g); break;
    }
    TNR_CHECK_LAUNCH("tnr_topk_scores");
    if (S > 1) {
        hipLaunchKernelGGL(topk_merge_kernel, dim3((unsigned)Nu), dim3(64), (size_t)S * K * 8, st, (const u64*)work, S, K, out_idx, out_score);
        TNR_CHECK_LAUNCH("tnr_topk_scores/merge");
    }
    return TNR_OK;
}
