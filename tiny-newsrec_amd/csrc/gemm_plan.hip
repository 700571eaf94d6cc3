// Host state and host arithmetic of the MFMA GEMMs (gemm.hip), shared by its bf16 and its fp16 build: the tile-queue counter sets,
// the routing by shape, the tilings of the persistent kernels - and the fp32 slab sums behind the weight gradients.
#include <algorithm>
#include <mutex>

#include "common.h"

// ---- routing ---------------------------------------------------------------------------------------
// Which kernel a launch takes depends on the shape only (and on the process-wide options of api.cpp, which tools set
// through tnr_gemm_set_option -- the library never reads the environment).  tnr_gemm_nt_route() exposes the decision
// so that the parity tests can pin every route.
int device_cus() {
    if (tnr_gemm_opts()->cus > 0) return tnr_gemm_opts()->cus;
    static int cus[64] = {0};
    int devid = 0;
    if (hipGetDevice(&devid) != hipSuccess || devid < 0 || devid >= 64) return 256;
    if (cus[devid] == 0) {
        hipDeviceProp_t prop;
        int n = 256;
        if (hipGetDeviceProperties(&prop, devid) == hipSuccess && prop.multiProcessorCount > 0) n = prop.multiProcessorCount;
        cus[devid] = n;
    }
    return cus[devid];
}

// Tiling of a ping-pong launch: instance (MI = 8: panels of 256 / 224 rows, MI = 7: 224 / 192), P row panels, x of them tall
// (pp_panel).  Cost model: a tile costs its rows + a fixed 24 (prologue latency, bias, queue), every XCD label's 1/8 of the tiles
// is pulled by 1/8 of the workgroups, a mixed launch pays half the height difference for the luck of the draw; candidates
// are all P between "all tall" and "all short".  mix = 0 (option `mix`, or column sums riding along: their partial rows
// are counted per 256-row panel, tnr_gemm_colsum_rows): the uniform tiling with the old 224 / 256 rule.
PpPlan pp_plan(int64_t M, int64_t N, int flags, int n_cu) {
    const TnrGemmOpts& o = *tnr_gemm_opts();
    const int64_t ncol = N / 256;
    if ((flags & TNR_EPI_COLSUM) || !o.mix) {
        const int64_t t256 = ((M + 255) / 256) * ncol, t224 = ((M + 223) / 224) * ncol;
        const int64_t c256 = ((t256 + n_cu - 1) / n_cu) * 256, c224 = ((t224 + n_cu - 1) / n_cu) * 224;
        bool use224 = c224 * 108 < c256 * 100 && !(flags & TNR_EPI_COLSUM);   // per-tile fixed costs: need a clear win
        if (o.bm) use224 = o.bm == 224 && !(flags & TNR_EPI_COLSUM);
        const int P = (int)(use224 ? (M + 223) / 224 : (M + 255) / 256);
        return PpPlan{use224 ? 7 : 8, P, P};
    }
    PpPlan best{8, (int)((M + 255) / 256), (int)((M + 255) / 256)};
    double best_span = 1e30;
    const int64_t W = n_cu >= 8 ? n_cu / 8 : 1;
    for (int mi = 8; mi >= 7; --mi) {
        if (o.bm && o.bm != 32 * mi) continue;
        const int tall = 32 * mi, shrt = tall - 32;
        const int64_t pmin = (M + tall - 1) / tall, pmax = (M + shrt - 1) / shrt;
        for (int64_t p = pmin; p <= pmax; ++p) {
            int64_t x = M - p * shrt;
            x = x > 0 ? (x + 31) / 32 : 0;                          // tall panels needed to cover M rows
            const double ct = tall + 24.0, cs = shrt + 24.0, f = (double)x / (double)p, cbar = f * ct + (1.0 - f) * cs;
            const int64_t n = (p * ncol + 7) / 8, k = n / W, r = n % W;
            double span = (double)k * cbar + (r ? cbar : 0.0) + (x > 0 && x < p ? 0.5 * (ct - cs) : 0.0);
            if (k == 0) span = x > 0 ? ct : cs;
            if (span < best_span - 1e-9) { best_span = span; best = PpPlan{mi, (int)p, (int)x}; }
        }
    }
    return best;
}

int nt_route(int64_t M, int64_t N, int64_t K, int flags, int n_cu) {
    const TnrGemmOpts& o = *tnr_gemm_opts();
    // 256x256 tiles: the persistent kernel, for N % 256 == 0 unless option "pp" = 0 rules out its tile queue
    const bool t256 = (N % 256) == 0 && o.pp;
    // short inputs (stage-1 title / body passes, small eval batches): when the 256x256 grid would leave more than 40 % of
    // the CUs without a tile, the 128x128 kernel (2 workgroups per CU) spreads the same work four times finer
    const bool sparse256 = t256 && ((M + 255) / 256) * (N / 256) * 100 < (int64_t)n_cu * o.fine_pct && !(flags & TNR_EPI_COLSUM);
    const bool odd_gelu = !t256 && (flags & (TNR_EPI_GELU | TNR_EPI_MULDGELU));   // the 256x128 kernel has no table GELU
    if (o.ver == 1 || M <= 128 || odd_gelu || (sparse256 && o.allow_fine)) return TNR_ROUTE_128x128;
    if (o.ver == 2 || !t256) return TNR_ROUTE_256x128;
    return pp_plan(M, N, flags, n_cu).mi == 7 ? TNR_ROUTE_224x256 : TNR_ROUTE_256x256;
}

// host-only (no HIP call): the tiling the persistent kernel would use on a device with n_cu compute units
extern "C" int tnr_gemm_nt_plan(int64_t M, int64_t N, int flags, int n_cu, int* mi, int* panels, int* tall) {
    TNR_CHECK_ARG(M >= 1 && N >= 256 && (N % 256) == 0 && n_cu >= 1 && mi && panels && tall, "tnr_gemm_nt_plan: bad argument");
    const PpPlan pl = pp_plan(M, N, flags, n_cu);
    *mi = pl.mi; *panels = pl.P; *tall = pl.x;
    return TNR_OK;
}

// Unit ranges of the eight XCD labels in a persistent weight-gradient launch (gemm.hip: TNGroup::xb): one problem -> equal unit counts (the old rule); several -> cut where the cumulated m steps (+ a fixed cost per
// unit for its prologue and slab store) reach x / 8 of the total
void tn_group_ranges(const int* ubase, const int* tiles_per_split, int n, int* xb) {
    const int total = ubase[TN_MAXP];
    if (n == 1) {
        const int q8 = total >> 3, r8 = total & 7;
        for (int x = 0; x <= 8; ++x) xb[x] = x < r8 ? x * (q8 + 1) : r8 * (q8 + 1) + (x - r8) * q8;
        return;
    }
    int64_t w[TN_MAXP], cum[TN_MAXP + 1];
    cum[0] = 0;
    for (int i = 0; i < n; ++i) {
        w[i] = tiles_per_split[i] + 8;
        cum[i + 1] = cum[i] + w[i] * (ubase[i + 1] - ubase[i]);
    }
    xb[0] = 0;
    xb[8] = total;
    for (int x = 1; x < 8; ++x) {
        const int64_t t = cum[n] * x / 8;
        int i = 0;
        while (i + 1 < n && cum[i + 1] <= t) ++i;
        int u = ubase[i] + (int)((t - cum[i] + w[i] / 2) / w[i]);
        if (u < xb[x - 1]) u = xb[x - 1];
        if (u > total) u = total;
        xb[x] = u;
    }
}

// Counter sets of the ping-pong kernel's tile queue (the ONE piece of device state the library keeps, include/tnr_hip.h):
// 128 sets in a __device__ array, one per (device, stream) the kernel has been launched on -- launches of a stream run in order,
// so each finds the set its predecessor returned to zero, and launches of different streams never share one.  A set is zeroed
// by a hipMemsetAsync on its stream when the stream is first bound and again by tnr_gemm_queue_reset(); every launch leaves
// it at zero (the last workgroup out resets it).  The table never drains a device and never changes the current device: when
// it is full the launch is refused (TNR_EUNSUPPORTED) and the caller either reuses fewer streams or runs with option "pp" = 0.
// ONE table for both builds of gemm.hip (bf16 and fp16), so a stream that launches kernels of both builds is bound once and
// tnr_gemm_queue_reset reaches the counters whichever build's kernel was aborted.
__device__ unsigned g_pp_queue[PP_QUEUE_SETS * PP_Q_SET];
unsigned* tnr_pp_queue_of(void* stream, bool reset) {
    hipStream_t st = (hipStream_t)stream;
    struct Slot { int dev; hipStream_t st; };
    static std::mutex mu;
    static Slot slots[PP_QUEUE_SETS];
    static int nslot = 0;
    static unsigned* base[64] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) { tnr_set_error("tnr_gemm_nt: no current device"); return nullptr; }
    std::lock_guard<std::mutex> lk(mu);
    if (!base[dev] && hipGetSymbolAddress((void**)&base[dev], HIP_SYMBOL(g_pp_queue)) != hipSuccess) {
        tnr_set_error("tnr_gemm_nt: tile-queue symbol not found");
        return nullptr;
    }
    unsigned* set = nullptr;
    for (int i = 0; i < nslot && !set; ++i)
        if (slots[i].dev == dev && slots[i].st == st) set = base[dev] + i * PP_Q_SET;
    const bool fresh = !set;
    if (!set) {
        if (nslot == PP_QUEUE_SETS) {
            tnr_set_error("tnr_gemm_nt: more than %d (device, stream) pairs have launched the persistent GEMM in this process "
                          "(reuse streams, or tnr_gemm_set_option(\"pp\", 0) for the kernels without a tile queue)", PP_QUEUE_SETS);
            return nullptr;
        }
        slots[nslot] = Slot{dev, st};
        set = base[dev] + (nslot++) * PP_Q_SET;
    }
    if ((fresh || reset) && hipMemsetAsync(set, 0, PP_Q_SET * sizeof(unsigned), st) != hipSuccess) {
        tnr_set_error("tnr_gemm_nt: could not zero the tile-queue counters");
        return nullptr;
    }
    return set;
}

// Zero the calling stream's tile-queue counters (stream-ordered).  Only needed after a launch on that stream was aborted (device
// fault, process-level recovery): a completed launch always leaves them at zero.
extern "C" int tnr_gemm_queue_reset(void* stream) {
    return tnr_pp_queue_of(stream, true) ? TNR_OK : TNR_EUNSUPPORTED;
}

// ---- slab sums of the weight gradients: dW (+)= out_scale * sum over the splits of the fp32 slabs ----------------
namespace {

__global__ void slab_reduce_kernel(const float* __restrict__ ws, int splits, int64_t NK, int K, float* out,
                                   int64_t ldo, int accumulate, float out_scale) {
    int64_t i4 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (i4 >= NK) return;
    f32x4 s = *(const f32x4*)(ws + i4);
    for (int z = 1; z < splits; ++z) s += *(const f32x4*)(ws + (int64_t)z * NK + i4);
    int64_t n = i4 / K, k = i4 - n * K;
    float* o = out + n * ldo + k;
    s *= out_scale;
    if (accumulate) s += *(const f32x4*)o;
    *(f32x4*)o = s;
}

// the slab sums of up to four problems in one launch (blockIdx.y = problem): each element exactly as slab_reduce_kernel does it
struct SlabGroup {
    const float* ws[TN_MAXP]; float* out[TN_MAXP]; int64_t NK[TN_MAXP], ldo[TN_MAXP];
    int splits[TN_MAXP], K[TN_MAXP], accumulate[TN_MAXP]; float out_scale[TN_MAXP];
};
__global__ void slab_reduce_group_kernel(SlabGroup g) {
    const int pi = blockIdx.y;
    const float* ws = g.ws[0]; float* out = g.out[0]; int64_t NK = g.NK[0], ldo = g.ldo[0];
    int splits = g.splits[0], K = g.K[0], accumulate = g.accumulate[0]; float out_scale = g.out_scale[0];
#pragma unroll
    for (int k = 1; k < TN_MAXP; ++k)
        if (pi == k) {
            ws = g.ws[k]; out = g.out[k]; NK = g.NK[k]; ldo = g.ldo[k];
            splits = g.splits[k]; K = g.K[k]; accumulate = g.accumulate[k]; out_scale = g.out_scale[k];
        }
    int64_t i4 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (i4 >= NK) return;
    f32x4 s = *(const f32x4*)(ws + i4);
    for (int z = 1; z < splits; ++z) s += *(const f32x4*)(ws + (int64_t)z * NK + i4);
    int64_t n = i4 / K, k = i4 - n * K;
    float* o = out + n * ldo + k;
    s *= out_scale;
    if (accumulate) s += *(const f32x4*)o;
    *(f32x4*)o = s;
}

}  // namespace

// launch only: the caller checks
void slab_reduce_launch(const SlabSum& s, hipStream_t st) {
    hipLaunchKernelGGL(slab_reduce_kernel, dim3((unsigned)((s.NK / 4 + 255) / 256)), dim3(256), 0, st, s.ws, s.splits, s.NK, s.K, s.out,
                       s.ldo, s.accumulate, s.out_scale);
}
void slab_reduce_group_launch(const SlabSum* s, int n, hipStream_t st) {
    SlabGroup g{};
    int64_t maxblk = 0;
    for (int i = 0; i < n; ++i) {
        g.ws[i] = s[i].ws; g.out[i] = s[i].out; g.NK[i] = s[i].NK; g.ldo[i] = s[i].ldo;
        g.splits[i] = s[i].splits; g.K[i] = s[i].K; g.accumulate[i] = s[i].accumulate; g.out_scale[i] = s[i].out_scale;
        maxblk = std::max<int64_t>(maxblk, (s[i].NK / 4 + 255) / 256);
    }
    hipLaunchKernelGGL(slab_reduce_group_kernel, dim3((unsigned)maxblk, (unsigned)n), dim3(256), 0, st, g);
}
