"""float64 reference of tnr_sgemm / tnr_sgemm_group (include/tnr_hip.h) and the case tables of tests/test_sgemm_kernels_gpu.py.

The contract, for z in [0, batch), m in [0, M), n in [0, N):
    C[c_off + z sC + m ldc + n] = alpha * sum_k A_z(m, k) B_z(n, k) + bias[bias_off + z sBias + n] + beta * (the element's old value)
    A_z(m, k) = A[a_off + z sA + m a_rs + k a_cs], likewise B;  nothing else is written;  beta == 0 does not read the destination.
A requested ksplit > 1 cuts K into `slices` slices of `kchunk` (effective_split) that are summed in slice order before alpha, bias
and beta are applied; part_elems floats of the caller's workspace hold the slices.

A problem is a dict with the field names of tnr_sgemm_problem_t.  A, B and bias are FLAT float32 numpy buffers and a_off, b_off,
bias_off, c_off are element offsets into them (into the destination for c_off), so strided, overlapping and offset views are
spelled exactly as the kernel sees them: pointer = buffer + offset, then the strides of the header.

The bound.  |fp32 result - float64| <= gamma_n (|alpha| sum_k |a||b| + |bias| + |beta c0|), gamma_n = n 2^-24 / (1 - n 2^-24),
n = K + slices + 3: the textbook bound of a fixed-order fp32 fma chain (tests/topk_ref.py uses the same convention) - at most K
roundings on any product, slices - 1 more where the slices are summed, three for alpha, bias and beta.  It is derived, not
measured, and holds for any order in which the MFMA adds its two k values."""
import numpy as np

FIELDS = ("A", "a_rs", "a_cs", "sA", "B", "b_rs", "b_cs", "sB", "C", "ldc", "sC", "bias", "sBias", "M", "N", "K", "batch", "alpha",
          "beta", "ksplit", "part")
SENT = -7.25
GUARD = 64


def _ceil(a, b):
    return -(-a // b)


def effective_split(K, ksplit):
    """-> (kchunk, slices) of a request for `ksplit` slices: the chunk is ceil(K / ksplit) rounded up to 16, and only as many
    slices as still hold a k are kept (a request the chunk rounding empties falls back to fewer, down to one unsplit pass)."""
    if ksplit <= 1:
        return K, 1
    kchunk = _ceil(_ceil(K, ksplit), 16) * 16
    return kchunk, _ceil(K, kchunk)


def part_elems(p):
    slices = effective_split(p["K"], p["ksplit"])[1]
    return slices * p["batch"] * p["M"] * p["N"] if slices > 1 else 0


def _index(off, s, rs, cs, Z, R, K):
    z, r, k = np.arange(Z)[:, None, None], np.arange(R)[None, :, None], np.arange(K)[None, None, :]
    return off + z * s + r * rs + k * cs


def operands(p):
    """-> A (batch, M, K), B (batch, N, K), bias (batch, N) in float64, and the flat destination index (batch, M, N)."""
    Z, M, N, K = p["batch"], p["M"], p["N"], p["K"]
    A = np.asarray(p["A"], np.float64)[_index(p["a_off"], p["sA"], p["a_rs"], p["a_cs"], Z, M, K)]
    B = np.asarray(p["B"], np.float64)[_index(p["b_off"], p["sB"], p["b_rs"], p["b_cs"], Z, N, K)]
    if p["bias"] is None:
        bias = np.zeros((Z, N))
    else:
        bias = np.asarray(p["bias"], np.float64)[p["bias_off"] + np.arange(Z)[:, None] * p["sBias"] + np.arange(N)[None, :]]
    return A, B, bias, _index(p["c_off"], p["sC"], p["ldc"], 1, Z, M, N)


def _finish(c_flat0, p, S, bias, ci, beta):
    want = np.asarray(c_flat0, np.float64).copy()
    v = p["alpha"] * S + bias[:, None, :]
    if beta != 0:
        v = v + beta * want[ci]
    want[ci] = v
    return want


def apply(c_flat0, p):
    """-> (want float64, bound float64, written bool), each as long as the flat destination c_flat0."""
    A, B, bias, ci = operands(p)
    assert ci.min() >= 0 and ci.max() < len(c_flat0) and len(np.unique(ci)) == ci.size, "the destination overlaps itself"
    want = _finish(c_flat0, p, np.einsum("zmk,znk->zmn", A, B), bias, ci, p["beta"])
    n = p["K"] + effective_split(p["K"], p["ksplit"])[1] + 3
    gamma = n * 2.0 ** -24 / (1.0 - n * 2.0 ** -24)
    mag = abs(p["alpha"]) * np.einsum("zmk,znk->zmn", np.abs(A), np.abs(B)) + np.abs(bias)[:, None, :]
    if p["beta"] != 0:
        mag = mag + np.abs(p["beta"] * np.asarray(c_flat0, np.float64)[ci])
    bound = np.zeros(len(c_flat0))
    bound[ci] = gamma * mag
    written = np.zeros(len(c_flat0), bool)
    written[ci] = True
    return want, bound, written


def mutants(p):
    """Yield (name, wrong) for every deliberately wrong reference that applies to p; wrong(c_flat0) -> float64 `want` of a kernel
    with that defect.  A test whose bound cannot tell these from apply() would not notice the defect either.
      drop_k           k index K // 2 is left out
      drop_last_pair   the last two k are left out (K >= 2)
      slice_overlap    the first k of every slice but the first is counted twice (split problems)
      bias_prev_batch  member z takes the bias of member z - 1, member 0 that of the last (batch > 1 with a bias)
      row_shift        row m takes A's row m + 1, the last row A's row 0 (M >= 2)
      beta_dropped     beta taken as 0 (beta != 0)
      ldc_is_N         the output laid out with N as its leading dimension (ldc > N, M >= 2)"""
    A, B, bias, ci = operands(p)
    Z, M, N, K = p["batch"], p["M"], p["N"], p["K"]
    kchunk, slices = effective_split(K, p["ksplit"])

    def make(A_=A, w=None, bias_=bias, beta=p["beta"], ci_=ci):
        w = np.ones(K) if w is None else w
        S = np.einsum("zmk,znk,k->zmn", A_, B, w)
        return lambda c_flat0: _finish(c_flat0, p, S, bias_, ci_, beta)

    w = np.ones(K)
    w[K // 2] = 0
    yield "drop_k", make(w=w)
    if K >= 2:
        w = np.ones(K)
        w[K - 2:] = 0
        yield "drop_last_pair", make(w=w)
    if slices > 1:
        w = np.ones(K)
        w[kchunk::kchunk] = 2
        yield "slice_overlap", make(w=w)
    if Z > 1 and p["bias"] is not None:
        yield "bias_prev_batch", make(bias_=np.roll(bias, 1, axis=0))
    if M >= 2:
        yield "row_shift", make(A_=np.roll(A, -1, axis=1))
    if p["beta"] != 0:
        yield "beta_dropped", make(beta=0.0)
    if p["ldc"] > N and M >= 2:
        yield "ldc_is_N", make(ci_=_index(p["c_off"], p["sC"], N, 1, Z, M, N))


# ------------------------------------------------------------------------------------------------ the cases
def _operand(rs, form, R, K, Z, shared):
    """One operand of R rows and K k values, Z batch members: -> (flat buffer, offset, row stride, k stride, batch stride).
    form: "k" k-fast rows, "k+5" k-fast rows of K + 5 (a padded row, hv.stride(0)), "r" row-fast (the transposed operand of dW =
    dY^T X), "g" a general stride pair (k stride 2, row stride 2 K + 3).  Every element of the buffer is random, also those no
    view reaches, so a wrong stride or offset reads wrong VALUES; members are 3 elements apart unless `shared` (batch stride 0)."""
    r_s, k_s = {"k": (K, 1), "k+5": (K + 5, 1), "r": (1, R), "g": (2 * K + 3, 2)}[form]
    span = (R - 1) * r_s + (K - 1) * k_s + 1
    off, s = 3, 0 if shared else span + 3
    buf = rs.standard_normal(off + (Z - 1) * s + span + 2).astype(np.float32)
    return buf, off, r_s, k_s, s


def make(M, N, K, batch=1, a="k", b="k", ldc_pad=0, c_gap=0, bias=False, bias_pad=0, alpha=1.0, beta=0.0, ksplit=1, shared_a=False,
         shared_b=False, c0=None, seed=0):
    """-> (problem, c_flat0).  The destination is [GUARD sentinels | body | GUARD sentinels] with c_off = GUARD; the body is the
    sentinel, N(0,1) values where beta != 0 (c0 "rand"), or NaN (c0 "nan")."""
    rs = np.random.RandomState(1000 + seed)
    A, a_off, a_rs, a_cs, sA = _operand(rs, a, M, K, batch, shared_a)
    B, b_off, b_rs, b_cs, sB = _operand(rs, b, N, K, batch, shared_b)
    p = dict(A=A, a_off=a_off, a_rs=a_rs, a_cs=a_cs, sA=sA, B=B, b_off=b_off, b_rs=b_rs, b_cs=b_cs, sB=sB, M=M, N=N, K=K, batch=batch,
             alpha=alpha, beta=beta, ksplit=ksplit, bias=None, bias_off=0, sBias=0)
    if bias:
        p.update(bias=rs.standard_normal(2 + batch * (N + bias_pad)).astype(np.float32), bias_off=2, sBias=N + bias_pad)
    p["ldc"] = N + ldc_pad
    p["sC"] = M * p["ldc"] + c_gap
    return p, destination(p, rs, c0 or ("rand" if beta != 0 else "sent"))


def destination(p, rs, c0):
    p["c_off"] = GUARD
    body = (p["batch"] - 1) * p["sC"] + (p["M"] - 1) * p["ldc"] + p["N"]
    c = np.full(body + 2 * GUARD, SENT, np.float32)
    if c0 == "rand":
        c[GUARD:GUARD + body] = rs.standard_normal(body)
    elif c0 == "nan":
        c[GUARD:GUARD + body] = np.nan
    return c


def make_score(C=5, D=36, Bn=4, seed=0):
    """stage1.py's score[b, c] = <title[b, c], body[b]>: A and B are views of ONE buffer X of Bn C title rows then Bn body rows,
    N = 1 and ldc = 1 (the members' C scores lie one behind the other)."""
    rs = np.random.RandomState(2000 + seed)
    X = rs.standard_normal((Bn * C + Bn) * D).astype(np.float32)
    p = dict(A=X, a_off=0, a_rs=D, a_cs=1, sA=C * D, B=X, b_off=Bn * C * D, b_rs=D, b_cs=1, sB=D, M=C, N=1, K=D, batch=Bn, alpha=1.0,
             beta=0.0, ksplit=1, bias=None, bias_off=0, sBias=0, ldc=1, sC=C)
    return p, destination(p, rs, "sent")


BASE = (33, 65, 65)
_EDGE_MN = (1, 31, 32, 33, 63, 64, 65, 129)
_EDGE_K = (1, 2, 3, 63, 64, 65, 127, 128, 129)
# (a) tile and k-step edges, unsplit, both operands k-fast; M = 48 has rows in both halves of a wave's 32 x 32 accumulator block
EDGE_SHAPES = sorted({(M, BASE[1], BASE[2]) for M in _EDGE_MN + (48,)} | {(BASE[0], N, BASE[2]) for N in _EDGE_MN} |
                     {(BASE[0], BASE[1], K) for K in _EDGE_K} | {(1, 1, 1), (1, 1, 129), (129, 1, 65), (1, 129, 65), (65, 65, 129)})
# (d) the requests of a split: (K, ksplit) -> the slices effective_split gives them
SPLIT_K = ((16, 8), (17, 8), (33, 2), (130, 2), (300, 8), (600, 8))
_FORMS = {"dW": dict(a="r", b="r"), "kfast": dict(a="k", b="k")}


def _table():
    t = {}
    for M, N, K in EDGE_SHAPES:
        t["edge/M%d_N%d_K%d" % (M, N, K)] = (make, dict(M=M, N=N, K=K))
    # (b) the four stride forms: forward (k, k), dW = dY^T X (r, r), dX = dY W (k, r), and A strided against B k-fast (r, k)
    for a in "kr":
        for b in "kr":
            for M, N, K in ((65, 33, 67), (33, 65, 130)):
                t["stride/A%s_B%s_M%d_N%d_K%d" % (a, b, M, N, K)] = (make, dict(M=M, N=N, K=K, a=a, b=b))
    t["stride/A_general_cs2_rs2K+3"] = (make, dict(M=33, N=65, K=67, a="g"))
    t["stride/A_padded_row_rsK+5"] = (make, dict(M=33, N=65, K=67, a="k+5"))
    # (c) the layouts the callers use
    t["layout/stage1_teacher_side_score_ldc1_N1"] = (make_score, dict())
    t["layout/engine_nrms_qkv_ldc_gap_batched_bias"] = (make, dict(M=35, N=48, K=40, batch=3, ldc_pad=5, c_gap=7, bias=True, bias_pad=3))
    t["layout/engine_user_epad_M1_batch2"] = (make, dict(M=1, N=36, K=40, batch=2, bias=True))
    t["layout/shared_A_sA0_batch3"] = (make, dict(M=33, N=65, K=65, batch=3, shared_a=True))
    t["layout/shared_B_sB0_batch3"] = (make, dict(M=33, N=65, K=65, batch=3, shared_b=True))
    t["layout/engine_dense_wgrad_accumulate_beta1"] = (make, dict(M=33, N=65, K=65, a="r", b="r", beta=1.0))
    t["layout/engine_dense_dgrad_alpha1024"] = (make, dict(M=33, N=65, K=65, a="k", b="r", alpha=1024.0))
    t["layout/beta0_over_nan"] = (make, dict(M=33, N=65, K=65, c0="nan"))
    t["layout/alpha_half_beta2_bias"] = (make, dict(M=33, N=65, K=65, batch=3, bias=True, alpha=0.5, beta=2.0))
    # (d) split-K; the K = 16 request falls back to one slice and still has to apply beta in the tile
    for K, ks in SPLIT_K:
        for form, kw in _FORMS.items():
            for Z in (1, 3):
                t["split/%s_K%d_ks%d_batch%d" % (form, K, ks, Z)] = (make, dict(M=33, N=65, K=K, batch=Z, ksplit=ks, beta=1.0 if K == 16 else 0.0, **kw))
    for form, kw in _FORMS.items():
        t["split/%s_K300_ks8_batch3_bias_alpha_beta_ldc_gap" % form] = (
            make, dict(M=33, N=65, K=300, batch=3, ksplit=8, bias=True, bias_pad=3, alpha=0.5, beta=2.0, ldc_pad=5, c_gap=7, **kw))
    return t


TABLE = _table()
CASES = sorted(TABLE)


def case(name):
    """-> (problem, c_flat0) of a table entry; the seed is the entry's position, so no two cases share data."""
    fn, kw = TABLE[name]
    return fn(seed=CASES.index(name), **kw)


# (f) the groups, by case name
GROUPS = {
    "one": ["edge/M33_N65_K65"],
    # tile grids gx x gy of 1x1, 3x1, 2x3, 2x2, 2x1 (batch 3, split), 1x1 (batch 3), 1x1 (M = 1, batch 2), 2x1 (batch 3, split)
    "eight": ["edge/M1_N1_K1", "edge/M33_N129_K65", "edge/M129_N65_K65", "edge/M65_N65_K129", "split/dW_K600_ks8_batch3",
              "layout/engine_nrms_qkv_ldc_gap_batched_bias", "layout/engine_user_epad_M1_batch2",
              "split/kfast_K300_ks8_batch3_bias_alpha_beta_ldc_gap"],
    "alternate": ["edge/M33_N65_K3", "split/dW_K17_ks8_batch1", "stride/Ak_Br_M65_N33_K67", "split/kfast_K130_ks2_batch3",
                  "split/dW_K300_ks8_batch3_bias_alpha_beta_ldc_gap", "layout/alpha_half_beta2_bias"],
    "fallback": ["edge/M65_N65_K65", "split/dW_K16_ks8_batch3", "stride/Ar_Bk_M33_N65_K130"],
}
