"""The MFMA GEMMs (csrc/gemm.hip, csrc/gemm_plan.hip), kernel by kernel and route by route, against the float64 references of
tests/gemm_ref.py (tied to the oracle, and its pinned tilings to the library, by tests/test_gemm_ref_cpu.py), at the smallest shapes
at which each path exists and in both 16-bit builds.

Routing is pinned through tnr_gemm_set_option ("ver", "bm", "allow_fine" = 0, "cus" = 8: the option sets of
tests/test_dropout_kernels_gpu.py), so no decision depends on the device's CU count; tnr_gemm_nt_route - and, on the persistent
routes, tnr_gemm_nt_plan - is asserted before every launch, and the options are back at their defaults after every test.

  * NT operands are over-allocated and poisoned: A (lda = K + 8) and B (ldb = K + 16) hold NaN in their gap columns, A, res (ldres =
    N + 4) and aux (ldaux = N + 12) NaN in the rows past M (the kernels clamp row reads to M - 1); C (ldc = N + 8, 8 rows past M)
    and the AUXOUT side output are prefilled with a sentinel that the gap columns and the rows past M must keep.
  * main loop: integer operands, flags 0 / OUTF32 / BIAS | RES, equal to float64 bit for bit, M off every row tile, K = 64, 128, 192,
    plus one launch per persistent instance with mixed panel heights and two rounds of its 8 workgroups - once more under "gm" = 2.
  * epilogues: every flag set the engine uses and three that land on the generic instance, random operands, against float64.
  * the GELU / GELU' tables swept through the bias (A = 0) and the aux operand: knots, mid-knots, the clamps, large |x|.
  * weight gradients: the three kernels at M = 1 .. 449 with every split rule, out_scale, accumulate, padded leading dimensions,
    NaN behind Mpad and in the workspace slabs past the effective split count; the grouped launch with a chain.
  * the tile queue: every persistent launch runs twice (equal bits); NT, weight gradient, NT back to back on one stream and side by
    side on two.
  * arguments the launchers refuse before any launch.

Bounds: tests/gemm_ref.py derives them (accumulation K 2^-24 sum|a||b|, one 16-bit rounding, the table's interpolation and erf
error, fixed-order sums); where the ceiling of tests/test_bench_shapes_gpu.py is tighter it applies.  Every test prints its largest
error and that error as a fraction of its bound (EXPERIMENTS.md item 62 records them)."""
import contextlib
import ctypes
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import gemm_ref as R                                          # noqa: E402
import tnr_hip as T                                           # noqa: E402
from test_dropout_kernels_gpu import ROUTE_ID, ROUTES         # noqa: E402

DEV = "cuda:0"
BUILDS = {"bf16": (torch.bfloat16, ""), "fp16": (torch.float16, "_f16")}
OPT_DEFAULTS = {"ver": 3, "gm": 8, "fine_pct": 60, "allow_fine": 1, "bm": 0, "pp": 1, "tnpp": 2, "mix": 1, "cus": 0}
PERSISTENT = {"224x256": 224, "256x256": 256}                 # route -> option "bm"
ROUTE_OPTS = {r: dict(o, **({"cus": R.PLAN_CUS} if r in PERSISTENT else {})) for r, o in ROUTES.items()}
NT_M = {"128x128": (1, 127, 129), "256x128": (129, 257), "224x256": (129, 225), "256x256": (129, 257)}
NT_N = {"128x128": (128, 384), "256x128": (128, 384), "224x256": (256, 768), "256x256": (256, 768)}
MIXED = {"224x256": (993, 768), "256x256": (1153, 768)}      # two tall panels among five, 15 tiles on 8 workgroups
KS = (64, 128, 192)
SENT = -7.25                                                  # exact in both 16-bit types
NAN = float("nan")
B_, G_, TH, R_, MD, F32O, AUX, CS = (R.EPI_BIAS, R.EPI_GELU, R.EPI_TANH, R.EPI_RES, R.EPI_MULDGELU, R.EPI_OUTF32, R.EPI_AUXOUT,
                                     R.EPI_COLSUM)
# TNR_PP_FLAG_SETS of csrc/gemm.hip without the dropout set, then three sets that take the generic (CF = -1) instance
FLAG_SETS = (0, B_, R_, B_ | R_, B_ | G_, B_ | G_ | AUX, MD, MD | CS, B_ | TH | F32O, B_ | F32O, R_ | F32O, B_ | TH)


@contextlib.contextmanager
def options(**kv):
    L_ = T.lib()
    try:
        for k, v in kv.items():
            assert L_.tnr_gemm_set_option(k.encode(), v) == 0
        yield
    finally:
        for k, v in OPT_DEFAULTS.items():
            L_.tnr_gemm_set_option(k.encode(), v)


def lib_plan(M, N, flags, n_cu):
    mi, P, x = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    ref = lambda v: ctypes.cast(ctypes.byref(v), ctypes.c_void_p)
    assert T.lib().tnr_gemm_nt_plan(M, N, flags, n_cu, ref(mi), ref(P), ref(x)) == 0
    return mi.value, P.value, x.value


class Report:
    """Largest error and worst error / bound per kind of comparison, printed once per test."""

    def __init__(self, test):
        self.test, self.rows = test, {}

    def check(self, kind, got, want, bound, what):
        got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
        assert got.shape == want.shape, what
        assert np.isfinite(got).all(), "%s: non-finite output" % (what,)
        err = np.abs(got - want)
        bound = np.broadcast_to(np.asarray(bound, np.float64), err.shape)
        ratio = np.where(err == 0.0, 0.0, err / np.maximum(bound, 1e-300))
        e, w = float(err.max(initial=0.0)), float(ratio.max(initial=0.0))
        pe, pw, n = self.rows.get(kind, (0.0, 0.0, 0))
        self.rows[kind] = (max(pe, e), max(pw, w), n + 1)
        assert (err <= bound).all(), "%s %s: %d of %d elements over the bound, max|err| %.3e, worst err / bound %.3f" % (
            kind, what, int((err > bound).sum()), err.size, e, w)

    def exact(self, kind, got, want, what):
        pe, pw, n = self.rows.get(kind, (0.0, 0.0, 0))
        self.rows[kind] = (pe, pw, n + 1)
        assert np.array_equal(np.asarray(got, np.float64), np.asarray(want, np.float64)), "%s %s: not bit-exact" % (kind, what)

    def done(self):
        for kind, (e, w, n) in sorted(self.rows.items()):
            print("[gemm-kernels] %s | %s: %d comparisons, max|err| %.3e, worst err / bound %.3f" % (self.test, kind, n, e, w))


def rnd(shape, seed, scale=1.0):
    return (np.random.RandomState(seed).standard_normal(shape) * scale).astype(np.float32)


def r16(x, td):
    """fp32 numpy -> the values the build's 16-bit type holds, as fp32 numpy."""
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(td).float().numpy()


def padded(x, extra_rows, ld, dt, fill=NAN):
    """x (r, c) -> device tensor (r + extra_rows, ld) of dtype dt holding x in [:r, :c] and `fill` everywhere else."""
    r, c = x.shape
    t = torch.full((r + extra_rows, ld), fill, dtype=dt)
    t[:r, :c] = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dt)
    return t.to(DEV)


def host(t):
    return t.float().cpu().numpy().astype(np.float64)


def bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def frame_kept(t, rows, cols):
    """the sentinel behind the (rows, cols) corner of a buffer prefilled with SENT (a value with one bit pattern)"""
    return bool((t[rows:] == SENT).all()) and bool((t[:, cols:] == SENT).all())


def expected_route(route, M, N, flags):
    """csrc/gemm_plan.hip: nt_route under the option set of `route`: M <= 128 always takes the 128x128 kernel; the 256x128 kernel
    has no table GELU, so it takes the GELU flags only under "ver" = 2 with N % 256 == 0 (its closed-form erf), an N that is no
    multiple of 256 sends them to the 128x128 kernel; column sums keep the 256-row instance of the persistent kernel."""
    if route == "128x128" or M <= 128:
        return T.ROUTE_128
    if route == "256x128":
        return T.ROUTE_128 if (flags & (G_ | MD)) and N % 256 else T.ROUTE_256x128
    if flags & CS:
        return T.ROUTE_256
    return ROUTE_ID[route]


# ------------------------------------------------------------------------------------------------ NT: operands and one launch
@functools.lru_cache(maxsize=None)
def int_operands(M, N, K):
    """Integer operands whose every output is an integer below 256 in magnitude (exact in bf16 and in fp16): entries in {-1, 0, 1}
    plus the asymmetry terms of tests/test_kernels_gpu.py (B[:, 0] += n % 5, A[:, 1] += m % 3: a row <-> column or tile swap cannot
    hide): |a b^T| <= K + 4 + 2 <= 198, integer bias in [-8, 8], integer residual in [-16, 16]: |C| <= 222."""
    rs = np.random.RandomState(M * 7 + N + K)
    A = rs.randint(-1, 2, (M, K)).astype(np.float32)
    B = rs.randint(-1, 2, (N, K)).astype(np.float32)
    B[:, 0] += np.arange(N) % 5
    A[:, 1] += np.arange(M) % 3
    bias = rs.randint(-8, 9, (N,)).astype(np.float32)
    res = rs.randint(-16, 17, (M, N)).astype(np.float32)
    return A, B, bias, res


@functools.lru_cache(maxsize=None)
def rnd_operands(dtype, M, N, K):
    """Random operands as the build's 16-bit type holds them: a ~ N(0, 1), b ~ N(0, 0.1^2), bias, res ~ N(0, 1), aux ~ N(0, 2^2)."""
    td = BUILDS[dtype][0]
    s = M * 11 + N * 3 + K
    return (r16(rnd((M, K), s), td), r16(rnd((N, K), s + 1, 0.1), td), rnd((N,), s + 2), r16(rnd((M, N), s + 3), td),
            r16(rnd((M, N), s + 4, 2.0), td))


class NT:
    """One NT problem on the device, poisoned as the module docstring says; run() launches it into fresh output buffers."""

    def __init__(self, dtype, M, N, K, a, b, bias=None, res=None, aux=None):
        self.dtype, (self.td, self.sfx) = dtype, BUILDS[dtype]
        self.M, self.N, self.K = M, N, K
        self.a = padded(a, 256, K + 8, self.td)
        self.b = padded(b, 0, K + 16, self.td)
        self.bias = torch.from_numpy(bias).to(DEV) if bias is not None else None
        self.res = padded(res, 8, N + 4, self.td) if res is not None else None
        self.aux_in = padded(aux, 8, N + 12, self.td) if aux is not None else None

    def route(self, flags):
        return T.query("tnr_gemm_nt_route" + self.sfx, self.M, self.N, self.K, flags)

    def run(self, flags):
        """-> (C (M + 8, N + 8), aux side output or None, column-sum partials (rows + 2, N) or None); no synchronisation."""
        M, N, K = self.M, self.N, self.K
        c = torch.full((M + 8, N + 8), SENT, device=DEV, dtype=torch.float32 if flags & F32O else self.td)
        aux = self.aux_in if flags & MD else (torch.full((M + 8, N + 12), SENT, device=DEV, dtype=self.td) if flags & AUX else None)
        cs = None
        if flags & CS:
            cs = torch.full((T.query("tnr_gemm_colsum_rows" + self.sfx, M) + 2, N), NAN, device=DEV)
            cs[-2:] = SENT
        res = self.res if flags & R_ else None
        T.call("tnr_gemm_nt_ex" + self.sfx, self.a, K + 8, self.b, K + 16, c, N + 8, M, N, K, self.bias if flags & B_ else None,
               res, N + 4 if res is not None else 0, aux, N + 12 if aux is not None else 0, flags, cs)
        return c, (aux if flags & AUX else None), cs


# rows summed into ONE column-sum partial row: nt_epilogue (128x128 and 256x128 kernels) writes one per 64-row strip of a wave
# (4 serial additions per lane, then a 4-level shuffle tree over 16 lanes); nt_epilogue_cols (persistent kernel) one per wave group
# of a 256-row tile, 8 blocks of 16 rows = 128 (rows 2 and 3 of a tile's four are zeros)
COLSUM_ROWS = {T.ROUTE_128: 64, T.ROUTE_256x128: 64, T.ROUTE_256: 128}


def assert_pinned(p, route, flags):
    want = expected_route(route, p.M, p.N, flags)
    assert p.route(flags) == want, (route, p.M, p.N, p.K, flags, p.route(flags), want)
    if want in (T.ROUTE_224, T.ROUTE_256):
        assert lib_plan(p.M, p.N, flags, R.PLAN_CUS) == R.plan(PERSISTENT[route], p.M, p.N, flags), (route, p.M, p.N, flags)
    return want


def run_twice(p, flags):
    """Two launches into fresh buffers: equal bits (the tile queue hands a launch's tiles out in an order that varies; a result
    may not), sentinels kept.  -> the first launch's buffers."""
    one, two = p.run(flags), p.run(flags)
    torch.cuda.synchronize()
    for x, y in zip(one, two):
        assert (x is None) == (y is None)
        if x is not None:
            assert torch.equal(bits(x), bits(y)), ("two runs differ", p.M, p.N, p.K, flags)
    c, aux, cs = one
    assert frame_kept(c, p.M, p.N), ("C: gap columns / rows past M written", p.M, p.N, p.K, flags)
    if aux is not None:
        assert frame_kept(aux, p.M, p.N), ("aux: gap columns / rows past M written", p.M, p.N, p.K, flags)
    if cs is not None:
        assert bool((cs[-2:] == SENT).all()), ("column sums: rows past tnr_gemm_colsum_rows(M) written", p.M, p.N, flags)
    return one


# ------------------------------------------------------------------------------------------------ NT: main loop
@pytest.mark.parametrize("dtype", list(BUILDS))
@pytest.mark.parametrize("route", list(ROUTES))
def test_nt_main_loop_integer_exact_on_every_route(route, dtype):
    """Integer operands (int_operands), flags 0, EPI_OUTF32 and EPI_BIAS | EPI_RES: every element equals float64 bit for bit.
    M per route: none a multiple of the row tile, 1 / 127 / 129 for the 128x128 kernel, one row past 128 (the smallest M the
    other routes take) and one row past their first row tile; N: 128 and 384 where N % 256 != 0 is allowed, 256 and 768 on the
    persistent routes; K: one, two and three 64-steps (a one-step main loop behind the multi-stage prologues; odd step counts for
    the kernels that unroll by two).  Persistent routes: also the mixed plan (MIXED: (7 | 8, 5, 2))."""
    rep = Report("main loop %s %s" % (route, dtype))
    with options(**ROUTE_OPTS[route]):
        shapes = [(M, N) for M in NT_M[route] for N in NT_N[route]] + ([MIXED[route]] if route in MIXED else [])
        for M, N in shapes:
            for K in KS:
                A, B, bias, res = int_operands(M, N, K)
                p = NT(dtype, M, N, K, A, B, bias, res)
                for flags in (0, F32O, B_ | R_):
                    assert_pinned(p, route, flags)
                    c, _, _ = run_twice(p, flags)
                    want, _ = R.linear(A, B, bias, res, flags=flags)
                    assert np.abs(want).max() < 256
                    rep.exact("C == float64", host(c[:M, :N]), want, (route, dtype, M, N, K, flags))
    rep.done()


# ------------------------------------------------------------------------------------------------ NT: epilogues
def nt_reference(p_ops, flags, K, dtype):
    """-> (out, pre, bound of pre in fp32, bound of the stored C), gemm_ref's derivations applied to one flag set:
      pre    (K + [bias]) 2^-24 (sum|a||b| + |bias|)
      GELU   the table is evaluated at the fp32 pre-activation v' = v + d: |GELU(v') - GELU(v)| <= sup|GELU'| d, the table's Phi is
             off by table_bound and multiplies |v'| <= |v| + d, the product is rounded once;
      tanh   slope <= 1, plus TANH_EVAL;
      GELU'  (MULDGELU) the factor GELU'(aux) carries d, the table's error multiplies |v'|, one rounding of the product;
      + res  one more fp32 addition: 2^-24 (|activation| + |res|);
    fp32 output: that bound alone; 16-bit output: round16_bound, or the ceiling of test_gemm_nt_epilogues_at_bench_shape where it
    is the tighter."""
    a, b, bias, res, aux = p_ops
    out, pre = R.linear(a, b, bias, res, aux, flags)
    d_pre = R.acc_bound(K, R.acc_mag(a, b, bias if flags & B_ else None), 1 if flags & B_ else 0)
    act, d = pre, d_pre
    if flags & G_:
        act = R.gelu(pre)
        d = R.GELU_SLOPE * d_pre + (np.abs(pre) + d_pre) * R.table_bound(pre, False) + R.U24 * np.abs(act)
    if flags & TH:
        act = np.tanh(pre)
        d = d_pre + R.TANH_EVAL
    if flags & MD:
        g = R.gelu_grad(aux)
        act = pre * g
        d = d_pre * np.abs(g) + (np.abs(pre) + d_pre) * R.table_bound(aux, True) + R.U24 * np.abs(act)
    if flags & R_:
        d = d + R.U24 * (np.abs(act) + np.abs(res))
    bound = d if flags & F32O else np.minimum(R.round16_bound(out, d, dtype), R.bench_ceiling(out, K, dtype))
    return out, pre, d_pre, bound


def check_nt_case(rep, route, p, ops, flags):
    """One launch (twice) of one flag set against float64: C, the AUXOUT side output (the rounded pre-activation), the column-sum
    partials (every row of tnr_gemm_colsum_rows(M) written over its NaN, their float64 sum = the column sums of the STORED C within
    the fixed-order bound of the rows one partial covers, COLSUM_ROWS)."""
    what = (route, p.dtype, p.M, p.N, p.K, flags)
    taken = assert_pinned(p, route, flags)
    c, aux, cs = run_twice(p, flags)
    out, pre, d_pre, bound = nt_reference(ops, flags, p.K, p.dtype)
    got = host(c[:p.M, :p.N])
    rep.check("C fp32" if flags & F32O else "C 16-bit", got, out, bound, what)
    if aux is not None:
        rep.check("aux side output", host(aux[:p.M, :p.N]), pre,
                  np.minimum(R.round16_bound(pre, d_pre, p.dtype), R.bench_ceiling(pre, p.K, p.dtype)), what)
    if cs is not None:
        parts = host(cs[:-2])
        assert np.isfinite(parts).all(), ("a column-sum partial row was not written", what)
        rep.check("column sums", parts.sum(0), got.sum(0), R.sum_bound(np.abs(got).sum(0), COLSUM_ROWS[taken]), what)
    return c


@pytest.mark.parametrize("dtype", list(BUILDS))
@pytest.mark.parametrize("route", list(ROUTES))
def test_nt_epilogues_against_float64_on_every_route(route, dtype):
    """FLAG_SETS on the shapes of the main-loop test (K = 64, 128 and 192), random operands.  Routing facts asserted on the way
    (expected_route): under the option set of the 256x128 route the GELU sets go to the 128x128 kernel at N = 128 / 384 and stay on
    the 256x128 kernel at N = 256, which is run for them as well; on the 224-row route a column-sum launch takes the 256-row
    instance.  EPI_COLSUM needs M > 128 (the launcher refuses it otherwise): on the 128x128 route it runs at M = 129 and at M = 257,
    three 128-row tiles, whose last two partial rows the launcher zeroes."""
    rep = Report("epilogues %s %s" % (route, dtype))
    with options(**ROUTE_OPTS[route]):
        shapes = [(M, N) for M in NT_M[route] for N in NT_N[route]] + ([MIXED[route]] if route in MIXED else [])
        for M, N in shapes:
            for K in KS:
                ops = rnd_operands(dtype, M, N, K)
                p = NT(dtype, M, N, K, *ops)
                for flags in FLAG_SETS:
                    if (flags & CS) and M <= 128:
                        continue
                    check_nt_case(rep, route, p, ops, flags)
        extra = {"128x128": [(257, 128, MD | CS), (257, 384, MD | CS)],
                 "256x128": [(M, 256, f) for M in NT_M[route] for f in (B_ | G_, B_ | G_ | AUX, MD, MD | CS)]}.get(route, [])
        for M, N, flags in extra:
            ops = rnd_operands(dtype, M, N, 128)
            check_nt_case(rep, route, NT(dtype, M, N, 128, *ops), ops, flags)
    rep.done()


@pytest.mark.parametrize("dtype", list(BUILDS))
@pytest.mark.parametrize("route", list(PERSISTENT))
def test_nt_mixed_plan_with_a_ragged_last_group_gives_the_same_bits(route, dtype):
    """The mixed plan's five row panels under "gm" = 2: groups of 2, 2 and 1 panels in the tile order (tile_coords), another
    assignment of tiles to workgroups and another order - the same bits as under "gm" = 8, with the full epilogue set of the engine's
    FFN launches."""
    rep = Report("gm = 2 %s %s" % (route, dtype))
    M, N = MIXED[route]
    ops = rnd_operands(dtype, M, N, 192)
    p = NT(dtype, M, N, 192, *ops)
    for flags in (B_ | G_ | AUX, B_ | R_, MD):
        outs = []
        for gm in (8, 2):
            with options(gm=gm, **ROUTE_OPTS[route]):
                c = check_nt_case(rep, route, p, ops, flags)
                outs.append(c)
        assert torch.equal(bits(outs[0]), bits(outs[1])), (route, dtype, flags)
    rep.done()


# ------------------------------------------------------------------------------------------------ the GELU tables
def table_grid():
    """The points of the sweep: every knot k / 128 of [-8, 8], every mid-knot, +-0, the fp32 subnormal 2^-130, the last knot below
    8 and the first step past it on both sides, and far outside the table: +-20, +-1e4."""
    knots = np.arange(-1024, 1025) / 128.0
    mids = (np.arange(-1024, 1024) + 0.5) / 128.0
    special = [0.0, -0.0, 2.0 ** -130, -2.0 ** -130, 7.9921875, -7.9921875, 8.0, -8.0, 8.0078125, -8.0078125, 20.0, -20.0, 1e4, -1e4]
    x = np.concatenate([knots, mids, special]).astype(np.float32)
    pad = (-len(x)) % 256
    return np.concatenate([x, np.zeros(pad, np.float32)])


@pytest.mark.parametrize("dtype", list(BUILDS))
@pytest.mark.parametrize("route", ["128x128", "224x256", "256x256"])
def test_table_gelu_and_its_derivative_swept_through_knots_clamps_and_large_x(route, dtype):
    """GELU: A = 0, so C = GELU_table(bias) and the fp32 bias IS x: EPI_BIAS | EPI_GELU (16-bit C) and, on the generic instance,
    | EPI_OUTF32 (the table's own error, no output rounding).  GELU': B = e_0 rows, A = 1.5 e_0, so A B^T = 1.5 exactly, and aux
    = the grid rounded to 16 bits: EPI_MULDGELU and | EPI_OUTF32.
    Every output is finite; a GELU output has the sign of x or is zero (Phi >= 0 in the table, so x Phi(x) cannot change sign);
    |GELU_table(x) - x Phi(x)| <= |x| table_bound + one fp32 rounding + fp32's subnormal floor (+ the 16-bit rounding), |1.5 GELU'_table(u) - 1.5 GELU'(u)|
    <= 1.5 table_bound + one rounding.  M = 129 on the persistent routes (their smallest), 2 on the 128x128 route."""
    rep = Report("tables %s %s" % (route, dtype))
    td, _ = BUILDS[dtype]
    x = table_grid()
    N, K, M = len(x), 64, (2 if route == "128x128" else 129)
    x64 = x.astype(np.float64)
    with options(**ROUTE_OPTS[route]):
        # ---- GELU of the bias
        p = NT(dtype, M, N, K, np.zeros((M, K), np.float32), r16(rnd((N, K), 5), td), bias=x)
        want = np.broadcast_to(R.gelu(x64), (M, N))
        d = np.abs(x64) * R.table_bound(x64, False) + R.U24 * np.abs(want) + R.FLOOR32
        for flags in (B_ | G_, B_ | G_ | F32O):
            assert_pinned(p, route, flags)
            c, _, _ = run_twice(p, flags)
            got = host(c[:M, :N])
            assert np.isfinite(got).all()
            sx = np.broadcast_to(np.sign(x64), got.shape)
            assert ((got == 0) | (np.sign(got) == sx)).all(), "a GELU output with the wrong sign"
            rep.check("GELU table" + (" fp32" if flags & F32O else " 16-bit"), got, want,
                      d if flags & F32O else R.round16_bound(want, d, dtype), (route, dtype, flags))
        # ---- GELU' of aux
        u = r16(x, td)
        u64 = u.astype(np.float64)
        a = np.zeros((M, K), np.float32)
        a[:, 0] = 1.5
        b = np.zeros((N, K), np.float32)
        b[:, 0] = 1.0
        p = NT(dtype, M, N, K, a, b, aux=np.broadcast_to(u, (M, N)))
        want = np.broadcast_to(1.5 * R.gelu_grad(u64), (M, N))
        d = 1.5 * R.table_bound(u64, True) + R.U24 * np.abs(want)
        for flags in (MD, MD | F32O):
            assert_pinned(p, route, flags)
            c, _, _ = run_twice(p, flags)
            rep.check("GELU' table" + (" fp32" if flags & F32O else " 16-bit"), host(c[:M, :N]), want,
                      d if flags & F32O else R.round16_bound(want, d, dtype), (route, dtype, flags))
    rep.done()


# ------------------------------------------------------------------------------------------------ weight gradients
WG_M = (1, 63, 64, 65, 129, 200, 449)
WG_SCALES = (1.0, 2.0 ** -7, 0.3)
# kernel -> (options, [(N, K)]): csrc/gemm.hip: tnr_gemm_tn_wgrad_ex picks by shape and option alone
WG_KERNELS = {
    "128-tile": ({}, [(128, 128), (384, 128)]),                     # N % 256 != 0
    "256x128": ({}, [(256, 128), (256, 384)]),                      # N % 256 == 0, K % 256 != 0
    "256x128 (tnpp = 0)": ({"tnpp": 0}, [(256, 256)]),
    "persistent": ({"tnpp": 2, "cus": R.PLAN_CUS}, [(256, 256), (256, 512)]),
}


@functools.lru_cache(maxsize=None)
def wg_operands(dtype, kind, N, K):
    """dY (449, N), X (449, K), dW0 (N, K) - integers (|dy| <= 3, |x| <= 4 with the asymmetry terms, so |dW| <= 12 M: exact in fp32
    whatever the order) or random - of which a case
    uses the first M rows."""
    td = BUILDS[dtype][0]
    M = max(WG_M)
    if kind == "int":
        rs = np.random.RandomState(N + 3 * K)
        dy, x = rs.randint(-2, 3, (M, N)).astype(np.float32), rs.randint(-2, 3, (M, K)).astype(np.float32)
        x[:, 0] += np.arange(M) % 3
        dy[:, 1] += np.arange(M) % 2
        return dy, x, rs.randint(-50, 51, (N, K)).astype(np.float32)
    return r16(rnd((M, N), N + K, 0.1), td), r16(rnd((M, K), N + K + 1), td), rnd((N, K), N + K + 2)


def wg_device(dtype, dy, x, M):
    """dY (lddy = N + 8) and X (ldx = K + 16): rows [M, Mpad) zero as include/tnr_hip.h requires, NaN in the 256 rows behind Mpad
    and in every gap column."""
    td = BUILDS[dtype][0]
    Mp = (M + 63) // 64 * 64
    out = []
    for t, gap in ((dy, 8), (x, 16)):
        z = np.zeros((Mp, t.shape[1]), np.float32)
        z[:M] = t[:M]
        out.append(padded(z, 256, t.shape[1] + gap, td))
    return out


def wg_run(dtype, dy_d, x_d, M, N, K, splits, acc, scale, dw0):
    """-> (dW (N + 4, K + 4) with a sentinel frame, ws: `splits` slabs prefilled with NaN); no synchronisation."""
    ws = torch.full((T.query("tnr_gemm_tn_ws_elems" + BUILDS[dtype][1], N, K, splits),), NAN, device=DEV)
    dW = torch.full((N + 4, K + 4), SENT, device=DEV)
    if acc:
        dW[:N, :K] = torch.from_numpy(dw0).to(DEV)
    T.call("tnr_gemm_tn_wgrad_ex" + BUILDS[dtype][1], dy_d, N + 8, x_d, K + 16, dW, K + 4, M, N, K, ws, splits, acc, scale)
    return dW, ws


def wg_bound(dy, x, M, scale, dw0, splits_eff):
    """M exact products accumulated in fp32 (M 2^-24), then the fixed-order slab sum, the scale and the accumulate (splits + 2 terms,
    gemm_ref.sum_bound's 2^-23 each), all relative to the sum of the terms' magnitudes."""
    return (M * R.U24 + (splits_eff + 2) * R.U23) * R.wgrad_mag(dy, x, M, scale, dw0)


def check_wgrad_case(rep, dtype, kind, N, K, M, splits, acc, scale, devs):
    dy, x, dw0 = wg_operands(dtype, kind, N, K)
    s32 = float(np.float32(scale))
    eff, _, _ = R.wgrad_splits(M, splits)
    what = (dtype, kind, N, K, M, splits, acc, scale)
    one = wg_run(dtype, *devs, M, N, K, splits, acc, s32, dw0)
    two = wg_run(dtype, *devs, M, N, K, splits, acc, s32, dw0)
    torch.cuda.synchronize()
    assert torch.equal(bits(one[0]), bits(two[0])), ("two runs differ", what)
    dW, ws = one
    assert frame_kept(dW, N, K), ("dW: gap columns / rows past N written", what)
    assert bool(torch.isfinite(ws[:eff * N * K]).all()), ("a live slab was not written", what)
    assert bool(torch.isnan(ws[eff * N * K:]).all()), ("a slab past the effective split count was written", what)
    want = R.wgrad(dy, x, M, s32, dw0 if acc else None)
    got = host(dW[:N, :K])
    if kind == "int" and scale != 0.3:
        rep.exact("dW == float64 (integers, out_scale a power of two)", got, want, what)
    else:
        rep.check("dW %s" % ("integers x 0.3" if kind == "int" else "random"), got, want,
                  wg_bound(dy, x, M, s32, dw0 if acc else None, eff), what)


@pytest.mark.parametrize("dtype", list(BUILDS))
@pytest.mark.parametrize("kernel", list(WG_KERNELS))
def test_wgrad_kernels_against_float64(kernel, dtype):
    """tnr_gemm_tn_wgrad_ex on each of its three kernels.  M = 1 .. 449 (1 to 8 tiles of 64 rows, ragged and not); splits 1, 2, 3, 7
    and 64 (clamped to the tile count; a tile count the split count does not divide gives a short last split: M = 449, 8 tiles, 3
    splits of 3, 3, 2 tiles; 5 splits become 4 of 2); accumulate 0 / 1 x out_scale 1, 2^-7, 0.3: all six for splits = 3 with integer
    and with random operands, one of the six in turn for the other split counts.  The workspace holds the caller's `splits` slabs of
    NaN: the live ones are overwritten, the others stay NaN and reach nothing."""
    rep = Report("wgrad %s %s" % (kernel, dtype))
    opts, shapes = WG_KERNELS[kernel]
    combos = [(acc, s) for acc in (0, 1) for s in WG_SCALES]
    with options(**opts):
        turn = 0
        for N, K in shapes:
            for M in WG_M:
                devs = {kind: wg_device(dtype, *wg_operands(dtype, kind, N, K)[:2], M) for kind in ("int", "rnd")}
                for splits in (1, 2, 3, 7, 64) + ((5,) if M == 449 else ()):
                    if splits == 3:
                        for acc, s in combos:
                            for kind in ("int", "rnd"):
                                check_wgrad_case(rep, dtype, kind, N, K, M, splits, acc, s, devs[kind])
                    else:
                        acc, s = combos[turn % len(combos)]
                        turn += 1
                        check_wgrad_case(rep, dtype, "int", N, K, M, splits, acc, s, devs["int"])
    rep.done()


def _group_problem(dtype, kind, N, K, M, splits, acc, scale, dW=None, ws_slabs=None):
    dy, x, dw0 = wg_operands(dtype, kind, N, K)
    dy_d, x_d = wg_device(dtype, dy, x, M)
    if dW is None:
        dW = torch.full((N + 4, K + 4), SENT, device=DEV)
        if acc == 1:
            dW[:N, :K] = torch.from_numpy(dw0).to(DEV)
    ws = torch.full((N * K * (ws_slabs or splits),), NAN, device=DEV) if acc != 2 else None
    q = dict(dY=dy_d, lddy=N + 8, X=x_d, ldx=K + 16, dW=dW, lddw=K + 4, M=M, N=N, K=K, ws=ws if ws is not None else 0,
             splits=splits, accumulate=acc, out_scale=float(np.float32(scale)))
    return q, (dy, x, dw0)


@pytest.mark.parametrize("dtype", list(BUILDS))
def test_wgrad_group_with_a_chain_against_float64_and_the_separate_calls(dtype):
    """tnr_gemm_tn_wgrad_group under "cus" = 8: four problems with different (M, splits) - a chained pair (accumulate = 2: two row
    ranges of one gradient, the head's workspace sized for the sum of the chain's `splits`), one with accumulate = 1, one with an
    out_scale - 13 units on 8 workgroups.  Against float64 within the bound; the unchained problems also bit for bit against their
    own tnr_gemm_tn_wgrad_ex calls.  The chained pair is compared with float64 only: separate calls would round the head's scaled
    sum before the second range is added, one slab sum over the chain does not, so equal bits do not follow by construction.
    Then a group with a (128, 128) problem, off the persistent route: the launcher's one-launch-per-problem path."""
    rep = Report("wgrad group %s" % dtype)
    f16 = dtype == "fp16"
    with options(tnpp=2, cus=R.PLAN_CUS):
        for kind in ("int", "rnd"):
            head, hops = _group_problem(dtype, kind, 256, 256, 449, 3, 0, 0.5, ws_slabs=3 + 2)
            tail, tops = _group_problem(dtype, kind, 256, 256, 200, 2, 2, 0.5, dW=head["dW"])
            p2, o2 = _group_problem(dtype, kind, 512, 256, 129, 7, 1, 1.0)
            p3, o3 = _group_problem(dtype, kind, 256, 512, 65, 1, 0, 2.0 ** -7)
            T.wgrad_group([head, tail, p2, p3], f16=f16)
            torch.cuda.synchronize()
            # the chain: rows [0, 449) of the head's operands and rows [0, 200) of the tail's (the same generator: the same rows)
            want = R.wgrad(hops[0], hops[1], 449, 0.5) + R.wgrad(tops[0], tops[1], 200, 0.5)
            mag = R.wgrad_mag(hops[0], hops[1], 449, 0.5) + R.wgrad_mag(tops[0], tops[1], 200, 0.5)
            got = host(head["dW"][:256, :256])
            assert frame_kept(head["dW"], 256, 256)
            if kind == "int":
                rep.exact("chain == float64 (integers)", got, want, (dtype, kind))
            else:
                rep.check("chain random", got, want, (649 * R.U24 + (3 + 2 + 2) * R.U23) * mag, (dtype, kind))
            assert bool(torch.isfinite(head["ws"]).all()), "the chain's five slabs are all live"
            for q, (dy, x, dw0), (N, K, M, splits, acc, scale) in ((p2, o2, (512, 256, 129, 7, 1, 1.0)), (p3, o3, (256, 512, 65, 1, 0, 2.0 ** -7))):
                eff = R.wgrad_splits(M, splits)[0]
                got = host(q["dW"][:N, :K])
                assert frame_kept(q["dW"], N, K)
                want = R.wgrad(dy, x, M, scale, dw0 if acc else None)
                if kind == "int":
                    rep.exact("group == float64 (integers)", got, want, (dtype, N, K, M))
                else:
                    rep.check("group random", got, want, wg_bound(dy, x, M, scale, dw0 if acc else None, eff), (dtype, N, K, M))
                solo, _ = wg_run(dtype, q["dY"], q["X"], M, N, K, splits, acc, float(np.float32(scale)), dw0)
                torch.cuda.synchronize()
                assert torch.equal(bits(solo), bits(q["dW"])), ("group != separate call", dtype, kind, N, K, M)
                assert bool(torch.isnan(q["ws"][eff * N * K:]).all())
        # ---- the fallback: a problem off the 256 x 256 route
        pa, oa = _group_problem(dtype, "rnd", 128, 128, 65, 2, 0, 1.0)
        pb, ob = _group_problem(dtype, "rnd", 256, 256, 129, 2, 1, 0.3)
        T.wgrad_group([pa, pb], f16=f16)
        torch.cuda.synchronize()
        for q, (dy, x, dw0), (N, K, M, splits, acc, scale) in ((pa, oa, (128, 128, 65, 2, 0, 1.0)), (pb, ob, (256, 256, 129, 2, 1, 0.3))):
            s32 = float(np.float32(scale))
            rep.check("fallback group random", host(q["dW"][:N, :K]), R.wgrad(dy, x, M, s32, dw0 if acc else None),
                      wg_bound(dy, x, M, s32, dw0 if acc else None, R.wgrad_splits(M, splits)[0]), (dtype, N, K, M))
            solo, _ = wg_run(dtype, q["dY"], q["X"], M, N, K, splits, acc, s32, dw0)
            torch.cuda.synchronize()
            assert torch.equal(bits(solo), bits(q["dW"])) and frame_kept(q["dW"], N, K)
    rep.done()


# ------------------------------------------------------------------------------------------------ the tile queue
@pytest.mark.parametrize("dtype", list(BUILDS))
def test_tile_queue_is_clean_between_launches_and_across_streams(dtype):
    """The persistent NT kernel and the persistent weight gradient share one counter set per stream, which every launch must leave
    at zero.  (a) NT (mixed plan, 15 tiles), weight gradient (8 tiles, 3 splits), NT (another shape and flag set) on one stream with
    no synchronisation in between: each result equals, bit for bit, that of the same launch run alone; (b) the first two side by
    side on two streams of their own (a counter set each): the same bits again."""
    M, N = MIXED["256x256"]
    ops1 = rnd_operands(dtype, M, N, 128)
    ops2 = rnd_operands(dtype, 257, 256, 64)
    dy, x, dw0 = wg_operands(dtype, "rnd", 256, 256)
    with options(tnpp=2, **ROUTE_OPTS["256x256"]):
        nt1, nt2 = NT(dtype, M, N, 128, *ops1), NT(dtype, 257, 256, 64, *ops2)
        wg_devs = wg_device(dtype, dy, x, 449)
        assert_pinned(nt1, "256x256", B_ | R_)
        assert_pinned(nt2, "256x256", B_ | G_ | AUX)
        steps = (lambda: nt1.run(B_ | R_)[:1], lambda: wg_run(dtype, *wg_devs, 449, 256, 256, 3, 1, 0.5, dw0)[:1],
                 lambda: nt2.run(B_ | G_ | AUX)[:2])
        solo = []
        for f in steps:
            solo.append(f())
            torch.cuda.synchronize()
        chained = [f() for f in steps]                       # back to back on the current stream
        torch.cuda.synchronize()
        for s, c in zip(solo, chained):
            for x_, y_ in zip(s, c):
                assert torch.equal(bits(x_), bits(y_)), "a launch behind another persistent launch differs from the same launch alone"
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        with torch.cuda.stream(s1):
            a_ = steps[0]()
        with torch.cuda.stream(s2):
            b_ = steps[1]()
        torch.cuda.synchronize()
        assert torch.equal(bits(a_[0]), bits(solo[0][0])) and torch.equal(bits(b_[0]), bits(solo[1][0])), "two streams"
        # and against float64, so that "equal" is not "equally wrong"
        rep = Report("tile queue %s" % dtype)
        out, _, _, bound = nt_reference(ops1, B_ | R_, 128, dtype)
        rep.check("NT behind nothing", host(solo[0][0][:M, :N]), out, bound, dtype)
        rep.check("wgrad between two NT launches", host(chained[1][0][:256, :256]), R.wgrad(dy, x, 449, 0.5, dw0),
                  wg_bound(dy, x, 449, 0.5, dw0, 3), dtype)
        rep.done()


# ------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize("dtype", list(BUILDS))
def test_launchers_refuse_bad_arguments_before_any_launch(dtype):
    """Arguments that csrc/gemm.hip's host checks reject (every TNR_CHECK_ARG of tnr_gemm_nt_do_split, tnr_gemm_tn_wgrad_ex and the
    head of tnr_gemm_tn_wgrad_group sits in front of the first launch): TnrError, and the output keeps its sentinel.  Every buffer
    is large enough for the call as if it were accepted."""
    td, sfx = BUILDS[dtype]
    M, N, K = 130, 256, 128
    a = torch.zeros((M + 8, K + 8), device=DEV, dtype=td)
    b = torch.zeros((N, K + 8), device=DEV, dtype=td)
    res = torch.zeros((M + 8, N + 8), device=DEV, dtype=td)
    c = torch.full((M + 8, N + 8), SENT, device=DEV, dtype=torch.float32)     # large enough for either output type
    cs = torch.full((16, N), SENT, device=DEV)
    bias = torch.zeros((N,), device=DEV)
    base = dict(a=a, lda=K + 8, b=b, ldb=K + 8, c=c, ldc=N + 8, M=M, N=N, K=K, bias=bias, res=res, ldres=N + 8, aux=res, ldaux=N + 8,
                flags=B_ | R_, cs=cs)
    bad_nt = {
        "lda % 8 != 0": dict(lda=K + 4),
        "ldc < N": dict(ldc=N - 4),
        "ldres % 4 != 0": dict(ldres=N + 2),
        "A off by 2 bytes": dict(a=a.view(-1)[1:]),
        "K = 32": dict(K=32),
        "N = 64": dict(N=64),
        "COLSUM with M = 128": dict(M=128, flags=MD | CS),
        "COLSUM | OUTF32": dict(flags=MD | CS | F32O),
        "EPI_DROPOUT as a flag": dict(flags=B_ | R_ | R.EPI_DROPOUT),
    }
    for name, change in bad_nt.items():
        q = dict(base, **change)
        with pytest.raises(T.TnrError):
            T.call("tnr_gemm_nt_ex" + sfx, q["a"], q["lda"], q["b"], q["ldb"], q["c"], q["ldc"], q["M"], q["N"], q["K"], q["bias"],
                   q["res"], q["ldres"], q["aux"], q["ldaux"], q["flags"], q["cs"])
        torch.cuda.synchronize()
        assert bool((c == SENT).all()) and bool((cs == SENT).all()), name
    # the accepted call, so that the refusals above are refusals of the one changed argument
    T.call("tnr_gemm_nt_ex" + sfx, a, K + 8, b, K + 8, c, N + 8, M, N, K, bias, res, N + 8, res, N + 8, B_ | R_ | F32O, None)
    torch.cuda.synchronize()
    assert bool((c[:M, :N] == 0).all()) and frame_kept(c, M, N)
    # ---- weight gradient
    Mw, Nw, Kw = 130, 128, 128
    dy = torch.zeros((192, Nw), device=DEV, dtype=td)
    x = torch.zeros((192, Kw), device=DEV, dtype=td)
    dW = torch.full((Nw, Kw), SENT, device=DEV)
    ws = torch.full((65 * Nw * Kw,), SENT, device=DEV)
    for name, (Kb, splits) in {"K = 64": (64, 2), "splits = 0": (Kw, 0), "splits = 65": (Kw, 65)}.items():
        with pytest.raises(T.TnrError):
            T.call("tnr_gemm_tn_wgrad_ex" + sfx, dy, Nw, x, Kw, dW, Kw, Mw, Nw, Kb, ws, splits, 0, 1.0)
        torch.cuda.synchronize()
        assert bool((dW == SENT).all()) and bool((ws == SENT).all()), name
    prob = lambda Nq, dWq, acc: dict(dY=torch.zeros((192, 512), device=DEV, dtype=td), lddy=512, X=torch.zeros((192, 256), device=DEV, dtype=td),
                                     ldx=256, dW=dWq, lddw=256, M=Mw, N=Nq, K=256, ws=torch.full((4 * Nq * 256,), SENT, device=DEV),
                                     splits=2, accumulate=acc, out_scale=1.0)
    dWg = torch.full((512, 256), SENT, device=DEV)
    groups = {"n = 0": [], "n = 5": [prob(256, dWg, 0) for _ in range(5)],
              "a chained problem whose N differs from its head's": [prob(256, dWg, 0), prob(512, dWg, 2)]}
    for name, g in groups.items():
        with pytest.raises(T.TnrError):
            T.wgrad_group(g, f16=dtype == "fp16")
        torch.cuda.synchronize()
        assert bool((dWg == SENT).all()), name
        assert all(bool((q["ws"] == SENT).all()) for q in g), name


# ------------------------------------------------------------------------------------------------ last: the defaults are back
def test_options_are_back_at_their_defaults():
    """Every test above restores OPT_DEFAULTS in a finally.  Under the defaults the headline step's attention-output launch (M =
    52 800, N = K = 768) tiles as include/tnr_hip.h says for 256 CUs - (7, 256, 114): "bm" = 0, "mix" = 1 - and takes the persistent
    route of that plan on this device ("ver" = 3, "pp" = 1, "cus" = 0); an N that is no multiple of 256 takes the 256x128 kernel."""
    assert lib_plan(52800, 768, 0, 256) == (7, 256, 114)
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    mi, _, _ = lib_plan(52800, 768, B_ | R_, n_cu)
    for sfx in ("", "_f16"):
        assert T.query("tnr_gemm_nt_route" + sfx, 52800, 768, 768, B_ | R_) == (T.ROUTE_224 if mi == 7 else T.ROUTE_256)
        assert T.query("tnr_gemm_nt_route" + sfx, 52800, 384, 768, B_) == T.ROUTE_256x128
        assert T.query("tnr_gemm_nt_route" + sfx, 52800, 384, 768, B_ | G_) == T.ROUTE_128
