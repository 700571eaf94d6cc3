"""float64 numpy restatements of what the MFMA GEMMs compute (csrc/gemm.hip, csrc/gemm_plan.hip) and the error bounds their tests
hold them to: the references of tests/test_gemm_kernels_gpu.py, tied to oracle/newsrec_oracle.py by tests/test_gemm_ref_cpu.py.
Nothing here is imported from the library; the epilogue flags are restated from include/tnr_hip.h.

Bounds (u = 2^-24, the unit roundoff of fp32; u16 = 2^-8 for bf16 and 2^-11 for fp16, one rounding of the stored output):
  * accumulation: the products of 16-bit operands are exact in fp32 (8 + 8 or 11 + 11 significant bits), so the only error of an
    fp32 dot product of K terms is that of its K - 1 additions, in whatever order: |err| <= K u sum|a||b|.  Every further fp32 addend
    of the epilogue (bias, residual) is one more term of the same sum: (K + n_extra) u (sum|a||b| + |bias| + |res|).
  * a 16-bit output stores round16(v') where v' is the fp32 value with error d from the float64 value v:
    |round16(v') - v| <= d + u16 |v'| <= u16 |v| + (1 + u16) d, plus the format's floor for results in its subnormal range.
  * the table GELU / GELU': see table_bound.
  * fixed-order fp32 sums (column sums, slab sums): count * 2^-23 * sum|terms|, the bound of tests/test_heads_kernels_gpu.py."""
import functools
import math

import numpy as np
from scipy.special import erf as _erf

F64 = np.float64
F32 = np.float32
U24 = 2.0 ** -24
U23 = 2.0 ** -23
EPI_BIAS, EPI_GELU, EPI_TANH, EPI_RES, EPI_MULDGELU, EPI_OUTF32, EPI_AUXOUT, EPI_COLSUM, EPI_DROPOUT = 1, 2, 4, 8, 16, 32, 64, 128, 256
U16 = {"bf16": 2.0 ** -8, "fp16": 2.0 ** -11}
# Results below the format's normal range: fp16 underflows gradually (subnormal spacing 2^-24, so half of it); bf16 shares fp32's
# exponent range, where the fp32 arithmetic in front of the conversion may itself flush: anything below the smallest normal number.
FLOOR16 = {"bf16": 2.0 ** -126, "fp16": 2.0 ** -25}
# fp32 results in fp32's own subnormal range (the table sweep feeds the kernels a subnormal bias): an instruction on the way may flush
FLOOR32 = 2.0 ** -126
LUT_STEP = 1.0 / 128.0                   # the table's step, over [-8, 8)
LUT_LO, LUT_HI = -8.0, 8.0
INV_SQRT2 = 0.70710678118654752
INV_SQRT_2PI = 0.39894228040143268


def f64(x):
    return np.asarray(x, F64)


# ------------------------------------------------------------------------------------------------ the operations
def phi(x):
    """The standard normal CDF."""
    return 0.5 * (1.0 + _erf(f64(x) / math.sqrt(2.0)))


def pdf(x):
    return np.exp(-0.5 * f64(x) ** 2) / math.sqrt(2.0 * math.pi)


def gelu(x):
    """erf-GELU (transformers BertIntermediate): x Phi(x)."""
    return f64(x) * phi(x)


def gelu_grad(x):
    """d GELU / dx = Phi(x) + x pdf(x)."""
    return phi(x) + f64(x) * pdf(x)


def linear(a, b, bias=None, res=None, aux=None, flags=0):
    """tnr_gemm_nt: pre = a b^T [+ bias], out = [GELU | tanh](pre) [* GELU'(aux)] [+ res]  ->  (out, pre), float64.
    a (M, K), b (N, K), bias (N,), res / aux (M, N).  The storage rounding (16-bit C, the 16-bit copy of pre that EPI_AUXOUT writes,
    the column sums of the ROUNDED C under EPI_COLSUM) is the caller's."""
    pre = f64(a) @ f64(b).T
    if flags & EPI_BIAS:
        pre = pre + f64(bias)[None, :]
    out = pre
    if flags & EPI_GELU:
        out = gelu(out)
    if flags & EPI_TANH:
        out = np.tanh(out)
    if flags & EPI_MULDGELU:
        out = out * gelu_grad(aux)
    if flags & EPI_RES:
        out = out + f64(res)
    return out, pre


def linear_bwd(dy, x, w):
    """Backward of y = x w^T + b for dy (M, N), x (M, K), w (N, K)  ->  (dx = dy w: tnr_gemm_nt with B = w^T, dw = dy^T x:
    tnr_gemm_tn_wgrad, db = column sums of dy: EPI_COLSUM of the launch that produced dy)."""
    return f64(dy) @ f64(w), wgrad(dy, x, len(dy)), f64(dy).sum(0)


def wgrad(dy, x, M, out_scale=1.0, dw0=None):
    """tnr_gemm_tn_wgrad_ex: dW (N, K) = [dw0 +] out_scale dy[:M]^T x[:M]."""
    dw = float(out_scale) * (f64(dy)[:M].T @ f64(x)[:M])
    return dw if dw0 is None else dw + f64(dw0)


def wgrad_mag(dy, x, M, out_scale=1.0, dw0=None):
    """sum of |terms| of wgrad: the scale of its rounding bound."""
    mag = abs(float(out_scale)) * (np.abs(f64(dy))[:M].T @ np.abs(f64(x))[:M])
    return mag if dw0 is None else mag + np.abs(f64(dw0))


# ------------------------------------------------------------------------------------------------ bounds
def acc_mag(a, b, bias=None, res=None):
    """sum |a||b| [+ |bias|] [+ |res|] per output element."""
    mag = np.abs(f64(a)) @ np.abs(f64(b)).T
    if bias is not None:
        mag = mag + np.abs(f64(bias))[None, :]
    if res is not None:
        mag = mag + np.abs(f64(res))
    return mag


def acc_bound(K, mag, n_extra=0):
    """fp32 accumulation of K exact products (+ n_extra further fp32 addends): (K + n_extra) 2^-24 sum|terms|."""
    return (K + n_extra) * U24 * f64(mag)


def round16_bound(want, d, dtype):
    """A 16-bit store of an fp32 value within d of `want`: u16 |want| + (1 + u16) d + the format's subnormal floor."""
    u = U16[dtype]
    return u * np.abs(f64(want)) + (1.0 + u) * f64(d) + FLOOR16[dtype]


def bench_ceiling(want, K, dtype):
    """The ceiling tests/test_bench_shapes_gpu.py::test_gemm_nt_epilogues_at_bench_shape holds 16-bit outputs to:
    rtol 2 eps, atol 2 eps + 2e-5 sqrt(K)."""
    eps = U16[dtype]
    return 2.0 * eps * np.abs(f64(want)) + 2.0 * eps + 2e-5 * math.sqrt(K)


def sum_bound(mag, count):
    """A fixed-order fp32 sum of `count` terms against the float64 sum: count * 2^-23 * sum|terms|."""
    return np.asarray(count, F64) * U23 * f64(mag)


# tnr_tanh (csrc/common.h): |x| < 0.06 -> x (1 - x^2 / 3 + 2 x^4 / 15), truncation 17 x^7 / 315 < 2e-10; else 1 - 2 / (E + 1) with
# E = __expf(2 x), relative error e_E <= 2^-22 (the hardware exp2 is good to 1 ulp, the product with log2 e adds |2 x| log2(e) u ln 2,
# and 2 E / (E + 1)^2 |2 x| < 0.5 damps it): d(2 / (E + 1)) = 2 E / (E + 1)^2 e_E <= 2^-23, the correctly rounded reciprocal, the
# doubling and the subtraction round values <= 2 once each: 3 x 2^-24 x 2.  Together < 8 x 2^-24.
TANH_EVAL = 8.0 * U24


def erf_as(z):
    """csrc/common.h: erf_as restated operation by operation in float32 (Abramowitz & Stegun 7.1.26); numpy's float32 exp and
    division stand in for __expf and __frcp_rn."""
    z = np.asarray(z, F32)
    a = np.abs(z)
    t = F32(1.0) / (F32(1.0) + F32(0.3275911) * a)
    e = np.exp(-a * a).astype(F32)
    p = t * (F32(0.254829592) + t * (F32(-0.284496736) + t * (F32(1.421413741) + t * (F32(-1.453152027) + t * F32(1.061405429)))))
    r = F32(1.0) - p * e
    return np.where(z < 0, -r, r).astype(F32), e


def lut_nodes(grad):
    """The node values lut_build (csrc/gemm.hip) computes, restated in float32: Phi(x_i) for GELU, GELU'(x_i) for its derivative,
    x_i = (i - 1024) / 128, i = 0 .. 2048 (the last one is only ever used as the right end of the last interval)."""
    x = ((np.arange(2049) - 1024).astype(F32) * F32(LUT_STEP)).astype(F32)
    r, e = erf_as(x * F32(INV_SQRT2))
    cdf = (F32(0.5) * (F32(1.0) + r)).astype(F32)
    if not grad:
        return x.astype(F64), cdf
    return x.astype(F64), (cdf + x * e * F32(INV_SQRT_2PI)).astype(F32)


def lut_node_error(grad):
    """max |restated node value - float64 value| over the table's nodes: the error of the erf approximation (and of its fp32
    evaluation) that fills the table.  tests/test_gemm_ref_cpu.py measures it and pins its size."""
    x, v = lut_nodes(grad)
    return float(np.abs(v.astype(F64) - (gelu_grad(x) if grad else phi(x))).max())


def _sup(fn, lo=LUT_LO, hi=LUT_HI, n=1 << 20):
    return float(np.abs(fn(np.linspace(lo, hi, n + 1))).max())


def table_bound(x, grad):
    """-> an array like x of the bound below (it does not depend on x).
    |table value at x - f(x)| for f = Phi (GELU(x) = x Phi(x): the caller multiplies by |x|) or f = GELU' (grad), the table of
    csrc/gemm.hip: lut_build / lut_eval.  Terms, all absolute:
      node      lut_node_error: the A&S approximation and its fp32 evaluation, measured on the restatement;
      fast exp  the device's __expf against the restatement's correctly rounded exp: <= 2 ulp of e <= 1, which reaches erf through
                p e with p <= 1 and Phi through the factor 0.5: 2^-23; GELU' adds x e / sqrt(2 pi) with |x e| <= e^-1/2: 2^-24;
      interp    linear interpolation over a step h = 1 / 128: h^2 / 8 max|f''| (Phi'' = -x pdf, GELU''' = x (x^2 - 4) pdf);
      index     t = fma(x, 128, 1024) is rounded to fp32: at most half an ulp of a number below 2048, 2^-14, i.e. the continuous
                piecewise-linear interpolant is evaluated 2^-21 away from x: max|f'| 2^-21 (Phi' = pdf, GELU'' = (2 - x^2) pdf);
                the node difference b - a is rounded too: 2^-24 of a number below max|f'| h;
      fma       the interpolation's one rounding of a value <= max|f| : 2^-24 max|f|.
    Outside [-8, 8) the index is clamped and the table returns an end value: f is within 1e-14 of its limits there (Phi(-8) =
    6e-16, |GELU'(-8)| = 1 - GELU'(8) = 4e-14), so the same bound holds with the end nodes' own error."""
    return np.full(f64(x).shape, _table_bound(bool(grad)))


@functools.lru_cache(maxsize=None)
def _table_bound(grad):
    if grad:
        d2 = _sup(lambda t: t * (t * t - 4.0) * pdf(t))
        d1 = _sup(lambda t: (2.0 - t * t) * pdf(t))
        fmax = _sup(gelu_grad)
        fast = 2.0 ** -23 + 2.0 ** -24
    else:
        d2 = _sup(lambda t: t * pdf(t))
        d1 = _sup(pdf)
        fmax = 1.0
        fast = 2.0 ** -23
    return lut_node_error(grad) + fast + LUT_STEP ** 2 / 8.0 * d2 + d1 * 2.0 ** -21 + U24 * d1 * LUT_STEP + U24 * fmax + 1e-13


GELU_SLOPE = 1.1289041451846717          # sup |GELU'| (at x = sqrt(2)); tests/test_gemm_ref_cpu.py checks it


# ------------------------------------------------------------------------------------------------ pinned tilings
# tnr_gemm_nt_plan(M, N, flags, n_cu = 8) -> (mi, panels, tall) under option "bm" = 224 / 256 (csrc/gemm_plan.hip: pp_plan), for
# every shape tests/test_gemm_kernels_gpu.py launches on a persistent route.  tests/test_gemm_ref_cpu.py asserts each entry with
# the library's host-only entry point, so the GPU file rests on a checked plan.  The two (5, 2) entries are the smallest launches
# with more than one round of the 8 workgroups and mixed panel heights: 15 tiles, two tall panels among five.
PLAN_CUS = 8
PLANS = {
    (224, 129, 256): (7, 1, 0), (224, 225, 256): (7, 2, 0), (224, 129, 768): (7, 1, 0), (224, 225, 768): (7, 2, 0),
    (224, 993, 768): (7, 5, 2), (224, 129, 4352): (7, 1, 0),
    (256, 129, 256): (8, 1, 0), (256, 257, 256): (8, 2, 0), (256, 129, 768): (8, 1, 0), (256, 257, 768): (8, 2, 0),
    (256, 1153, 768): (8, 5, 2), (256, 129, 4352): (8, 1, 0),
}


def plan(bm, M, N, flags):
    """The pinned tiling; column sums ride on the uniform 256-row tiling whatever "bm" says (their partial rows are counted per
    256-row panel, tnr_gemm_colsum_rows)."""
    if flags & EPI_COLSUM:
        p = (M + 255) // 256
        return (8, p, p)
    return PLANS[(bm, M, N)]


def panel_rows(M, mi, panels, tall):
    """[(first row, height)] of the row panels of a plan (include/tnr_hip.h: panel p starts at (32 mi - 32) p + 32 floor(p tall /
    panels) and is tall iff floor((p + 1) tall / panels) > floor(p tall / panels))."""
    out = []
    for p in range(panels):
        a, b = (p * tall) // panels, ((p + 1) * tall) // panels
        out.append(((32 * mi - 32) * p + 32 * a, 32 * mi if b > a else 32 * mi - 32))
    return out


def wgrad_splits(M, splits):
    """The effective split count of tnr_gemm_tn_wgrad_ex: `splits` clamped to the number of 64-row tiles, then the number of
    non-empty splits of ceil(tiles / splits) tiles each  ->  (effective splits, tiles per split, tiles)."""
    mt = (M + 63) // 64
    s = min(splits, mt)
    tps = (mt + s - 1) // s
    return (mt + tps - 1) // tps, tps, mt
