"""float64 reference, elementwise bounds, a float32 rounding model and the case table of the attention kernels (csrc/attn.hip:
tnr_attn_l32_fwd / _bwd, tnr_attn_long_fwd / _bwd), for tests/test_attn_ref_cpu.py (no GPU: the bounds are satisfiable and not
slack, every seeded defect of the model is caught) and tests/test_attn_kernels_gpu.py (the kernels themselves).

Inputs are the 16-bit-rounded values the kernel sees (rows_ref.r16); the reference is dropout_ref.attn_fwd / attn_bwd in float64
plus the inner matrices (S, dP, delta) they do not return.  mask_add is (N, Lp) and rel (A, Lp, Lp), Lp = 32 for the l32 form and
roundup(L, 32) for the long one, with -1e30 in mask_add's columns >= L and 0 in rel's rows / columns >= L, as tnr_embed_ln_fwd and
tnr_relpos_table write them (include/tnr_hip.h): the kernels read those cells.

Where the kernels round (line numbers of csrc/attn.hip), u = rows_ref.U16, tiny = rows_ref.TINY16, U23 = 2^-23:
  scores    fp32 MFMA sums over the 64 products of a head, * 0.125 (exact), + mask, + rel: l32 :106-114 / :222-232 / :284-297,
            long :450-457 / :598-608 / :704-716.   e_s = U23 (64 sum|q||k| / 8 + 2 (|q.k| / 8 + |mask| + |rel|)): at a padded key
            (mask -10000) fp32 is spaced 2^-10 and the two additions alone move a score by up to 1e-3.
  lse       max + __logf(sum of __expf): :263, :494.  d lse <= sum_k p_k e_s_k (the scores) + 1e-4 (1 + |log l|) (the relative
            ceiling FWD of tests/test_heads_kernels_gpu.py behind __expf - on l, so absolute on log l - and behind __logf) + U23 |lse|
            (the last addition).  The bound is min(1e-4 |lse|, that) + the score term: never above 1e-4 |lse| + the score term, and
            on an all-pad row (|lse| = 10000) a thousand times below it - at 1e-4 |lse| = 1 no output of this file would notice
            a wrong lse there.
  p         relative error rp_f = e_s + sum_k p_k e_s_k + 2e-4 in the forward kernels (exp(s - max) / sum, :123-129, or exp(s - running
            max) with the normaliser summed from the unrounded values, :468-472: two __expf ceilings, no __logf) and rp = e_s + d lse +
            1e-4 in the backward ones (exp(s - lse) behind the fp32 lse, :297, :608, :716).
  P         rounded to 16 bits: l32 normalised (:140 acc_to_frags, :312), long UNNORMALISED (:484; <= 1, scaled by <= 1 afterwards,
            so its absolute part stays below tiny) and per key tile in backward (:722).  b_P = (u + rp) p + tiny, rp_f for rp in the forward.
  ctx       fp32 sums of P16 v (:148, :490; the long form rescales O by exp(m_old - m_new) per tile, :488, and by 1 / l, :501),
            rounded to 16 bits (:59 acc_to_lds, :501):  u |ctx| + tiny + sum_j b_P_ij |v_j| + (L + 2 tiles + 4) U23 sum_j p_ij |v_j|.
  dP        fp32 MFMA over 64 products (:223, :285, :599, :705): e_dP = 64 U23 sum_d |dO||v|.
  delta     l32: sum_j p_ij dP_ij over the UNROUNDED p (:259), no ctx term.  long: sum_d dO O over the stored 16-bit ctx (:548), so
            d delta_i <= sum_d |dO_id| b_ctx_id + 66 U23 sum_d |dO||ctx|.
  dS        p (dP - delta) rounded to 16 bits (:270, :313, :613, :723): u |dS| + tiny + rp |dS| + p (e_dP + d delta) + 2 U23 p (|dP| +
            |delta|).
  dq, dk    fp32 sums of dS16 k (dS16^T q), * 0.125, rounded (:349-352, :621, :735): sum_j b_dS |k_j| / 8 + (L + 2) U23 sum |dS||k| / 8
            under the output rounding u |dq| + tiny.   dv: the same over b_P and dO (:321, :728, :353, :737).
No flat floor, no element skipped.  The bounds are worst-case sums; the sharp check is the aggregate one: the Frobenius norm of an
output's error against twice that of emulate() on the same inputs.

Cases: the table below is the only list of shapes (both test files read it).  Input kinds: plain, pad30, allpad, leftpad (keys
0 .. 31 padded), lastreal (only key L - 1 real), lastdom / firstdom (one key holds p >= 0.5 for every query), rising / falling (+6 /
-6 per 32-key tile on the mask of the real keys), sharp (q x 3), dspike (dO concentrated on one column per row: the one case where
delta's sum over 64 columns does not average the roundings it inherits from ctx, so that its worst-case bound is approached).

emulate(kind, form, inp) is a numpy float32 model of each kernel with r16 at exactly the points above (the long forward tile by
tile with its running max, the backward kernels in both orientations) and __expf / __logf as the device library evaluates them
(exp2(x log2 e), log2(x) ln 2 in fp32); it never stands in for the reference.  defect= seeds one slip (DEFECTS) for the CPU
file's mutant test.  failures() is the one list of checks both files apply to a set of outputs."""
import collections

import numpy as np

import dropout_ref as DR
import rows_ref as RR
from oracle import newsrec_oracle as O

F64, F32 = np.float64, np.float32
D = 64
U23 = RR.U23
FWD = RR.FWD                                   # 1e-4: the relative ceiling behind __expf / __logf
MARGIN = 2.0                                   # ||got - ref||_F <= MARGIN ||emulate - ref||_F
PAD, NEG_INF = -10000.0, -1e30
NEG_BIG = F32(-3.0e38)
SENT = -7.25
OUTS = ("ctx", "lse", "delta", "dq", "dk", "dv")

Case = collections.namedtuple("Case", "form N L A inp")
# every L with one (N, A), every (N, A) with two Ls, A = 12 once; pair counts N A = 1, 2, 3, 5, 9 (and 12)
L32_CASES = [Case("l32", *c) for c in (
    (1, 1, 1, "plain"), (1, 2, 2, "pad30"), (1, 4, 3, "plain"), (5, 5, 1, "lastdom"), (3, 8, 3, "pad30"), (1, 9, 1, "firstdom"),
    (1, 16, 2, "sharp"), (5, 17, 1, "allpad"), (3, 31, 3, "lastdom"), (1, 32, 3, "plain"), (1, 31, 12, "pad30"), (5, 9, 1, "plain"))]
LONG_CASES = [Case("long", *c) for c in (
    (1, 1, 1, "plain"), (2, 24, 2, "pad30"), (1, 32, 3, "plain"), (2, 33, 1, "lastdom"), (1, 33, 12, "plain"), (1, 64, 2, "leftpad"),
    (2, 97, 1, "lastreal"), (1, 97, 3, "sharp"), (2, 128, 1, "rising"), (2, 129, 2, "lastdom"), (1, 129, 1, "allpad"),
    (1, 160, 3, "falling"), (2, 200, 1, "leftpad"), (1, 200, 2, "firstdom"), (1, 256, 1, "rising"), (2, 160, 1, "allpad"),
    (1, 481, 1, "pad30"), (1, 24, 1, "dspike"))]
CASES = L32_CASES + LONG_CASES
DEFECTS = {  # defect -> the case designed for it
    "unmasked_pad": Case("long", 2, 129, 2, "lastdom"), "skip_rescale": Case("long", 2, 128, 1, "rising"),
    "stale_l": Case("long", 2, 128, 1, "rising"), "rel_T_long": Case("long", 1, 97, 3, "sharp"),
    "rel_T_l32": Case("l32", 3, 31, 3, "lastdom"), "dk_no_scale": Case("long", 2, 33, 1, "lastdom"),
    "dO_pad_long": Case("long", 2, 129, 2, "lastdom"), "dO_pad_l32": Case("l32", 5, 17, 1, "allpad"),
    "perm": Case("l32", 3, 8, 3, "pad30"), "perm_long": Case("long", 1, 160, 3, "falling"),
    "bias_row": Case("l32", 5, 5, 1, "lastdom"), "spare_l32": Case("l32", 5, 9, 1, "plain"),
    "spare_long": Case("long", 1, 129, 1, "allpad")}


def case_id(c):
    return "%s-N%d-L%d-A%d-%s" % c


def pitch(form, L):
    return 32 if form == "l32" else (L + 31) // 32 * 32


def heads(x, N, L, A):
    return np.asarray(x).reshape(N, L, A, D).transpose(0, 2, 1, 3)


def rows(x):
    N, A, L, _ = x.shape
    return x.transpose(0, 2, 1, 3).reshape(N * L, A * D)


# ------------------------------------------------------------------------------------------------ inputs
def inputs(c, kind, seed=0):
    """-> dict(qkv (N L, 3 A 64), dctx (N L, A 64): float64 of the 16-bit-rounded values; mask_add (N, Lp), rel (A, Lp, Lp): fp32)."""
    form, N, L, A, inp = c
    Lp = pitch(form, L)
    rs = np.random.RandomState(1000 * L + 10 * N + A + seed)
    q, k, v = [rs.standard_normal((N, L, A, D)) for _ in range(3)]
    dctx = rs.standard_normal((N * L, A * D))
    w = (rs.standard_normal((A, 32)) * 0.5).astype(F32)
    real = np.zeros((N, L))
    if inp == "pad30":
        real[rs.rand(N, L) < 0.3] = PAD
    elif inp == "allpad":
        real[:] = PAD
    elif inp == "leftpad":
        real[:, :32] = PAD
    elif inp == "lastreal":
        real[:, :L - 1] = PAD
    elif inp in ("rising", "falling"):
        real += (6.0 if inp == "rising" else -6.0) * (np.arange(L) // 32)
    elif inp in ("lastdom", "firstdom"):
        # every query carries a common direction of norm 4 beside half its noise, and the dominant key is 6 times that direction:
        # its score is 6 (16 +- 2 sigma) / 8 against N(0, 0.7) for the others
        dirn = rs.standard_normal((N, 1, A, D))
        dirn *= 4.0 / np.linalg.norm(dirn, axis=-1, keepdims=True)
        q = 0.5 * q + dirn
        k[:, L - 1 if inp == "lastdom" else 0] = 6.0 * dirn[:, 0]
    elif inp == "sharp":
        q = 3.0 * q
    elif inp == "dspike":
        # dO of row i is 4 e_(i mod 64) beside a hundredth of its noise: delta_i = sum_d dO_id O_id has one term that counts, so what
        # delta inherits from the stored ctx is not averaged over 64 columns and its worst-case bound is met to within a factor 3
        dctx = 0.01 * dctx
        for i in range(L):
            dctx.reshape(N, L, A, D)[:, i, :, i % D] += 4.0
    else:
        assert inp == "plain", inp
    qkv = np.concatenate([x.reshape(N * L, A * D) for x in (q, k, v)], 1)
    mask_add = np.full((N, Lp), NEG_INF, F32)
    mask_add[:, :L] = real
    rel = np.zeros((A, Lp, Lp), F32)
    rel[:, :L, :L] = O.relpos_bias_table(w, L)
    return dict(qkv=RR.r16(qkv, kind), dctx=RR.r16(dctx, kind), mask_add=mask_add, rel=rel, dims=(N, L, A), form=form)


# ------------------------------------------------------------------------------------------------ float64 reference
def reference(inp):
    """-> q, k, v, dO (N, A, L, 64); S, P, dP, dS (N, A, L, L); lse, delta (N, A, L); ctx, dq, dk, dv (N, A, L, 64); colsum (N, 3 A 64)
    = the per-sequence column sums of dqkv."""
    N, L, A = inp["dims"]
    madd, rel = inp["mask_add"][:, :L].astype(F64), inp["rel"][:, :L, :L].astype(F64)
    c = DR.attn_fwd(inp["qkv"], madd, rel, N, L, A)
    dqkv, ds = DR.attn_bwd(c, inp["dctx"])
    q, k, v, p = c["q"], c["k"], c["v"], c["p"]
    dO = heads(inp["dctx"], N, L, A)
    S = q @ k.transpose(0, 1, 3, 2) / 8.0 + madd[:, None, None, :] + rel[None]
    dP = dO @ v.transpose(0, 1, 3, 2)
    HD = A * D
    return dict(q=q, k=k, v=v, dO=dO, S=S, P=p, lse=c["lse"], ctx=heads(c["ctx"], N, L, A), dP=dP, delta=(dP * p).sum(-1), dS=ds,
                dq=heads(dqkv[:, :HD], N, L, A), dk=heads(dqkv[:, HD:2 * HD], N, L, A), dv=heads(dqkv[:, 2 * HD:], N, L, A),
                colsum=dqkv.reshape(N, L, 3 * HD).sum(1), madd=madd, rel=rel)


def bounds(r, kind, form):
    """Elementwise bounds of ctx, lse, delta, dq, dk, dv (the reference's layouts) and of the inner P and dS; see the module docstring."""
    u, tiny = RR.U16[kind], RR.TINY16[kind]
    T_ = lambda x: x.transpose(0, 1, 3, 2)
    q, k, v, dO, p, dS, dP = r["q"], r["k"], r["v"], r["dO"], r["P"], r["dS"], r["dP"]
    aq, ak, av, ad = np.abs(q), np.abs(k), np.abs(v), np.abs(dO)
    L = q.shape[2]
    tiles = (L + 31) // 32
    e_s = U23 * (64 * (aq @ T_(ak)) / 8.0 + 2 * (np.abs(q @ T_(k)) / 8.0 + np.abs(r["madd"])[:, None, None, :] + np.abs(r["rel"])[None]))
    es_row = (p * e_s).sum(-1)
    logl = r["lse"] - r["S"].max(-1)
    d_lse = FWD * (1 + np.abs(logl)) + U23 * np.abs(r["lse"]) + es_row
    b_lse = np.minimum(FWD * np.abs(r["lse"]), FWD * (1 + np.abs(logl)) + U23 * np.abs(r["lse"])) + es_row
    rp = e_s + d_lse[..., None] + FWD                       # backward: exp(s - lse) behind the stored lse
    rp_f = e_s + es_row[..., None] + 2 * FWD                # forward: exp(s - max) / sum, no __logf and no stored lse in between
    b_P, b_Pf = (u + rp) * p + tiny, (u + rp_f) * p + tiny
    fp_ctx = (L + 2 * tiles + 4) * U23 * (p @ av)
    b_ctx = RR.out16(r["ctx"], kind, b_Pf @ av + fp_ctx)
    e_dP = 64 * U23 * (ad @ T_(av))
    if form == "long":
        b_delta = (ad * b_ctx).sum(-1) + 66 * U23 * (ad * np.abs(r["ctx"])).sum(-1)
    else:
        b_delta = (rp * p * np.abs(dP) + p * e_dP).sum(-1) + (L + 2) * U23 * (p * np.abs(dP)).sum(-1)
    b_dS = (u + rp) * np.abs(dS) + tiny + p * (e_dP + b_delta[..., None]) + 2 * U23 * p * (np.abs(dP) + np.abs(r["delta"])[..., None])
    b_dq = RR.out16(r["dq"], kind, (b_dS @ ak + (L + 2) * U23 * (np.abs(dS) @ ak)) / 8.0)
    b_dk = RR.out16(r["dk"], kind, (T_(b_dS) @ aq + (L + 2) * U23 * (T_(np.abs(dS)) @ aq)) / 8.0)
    b_dv = RR.out16(r["dv"], kind, T_(b_P) @ ad + (L + 1) * U23 * (T_(p) @ ad))
    return dict(ctx=b_ctx, lse=b_lse, delta=b_delta, dq=b_dq, dk=b_dk, dv=b_dv, P=b_P, P_fwd=b_Pf, dS=b_dS)


# ------------------------------------------------------------------------------------------------ the float32 rounding model
def _expf(x):
    with np.errstate(over="ignore"):           # -3e38 log2 e = -inf -> 0, as on the device
        return np.exp2((x.astype(F32) * F32(1.4426950408889634)).astype(F32)).astype(F32)


def _logf(x):
    return (np.log2(x.astype(F32)).astype(F32) * F32(0.6931471805599453)).astype(F32)


def _swap48(x):
    """keys 0..3 and 4..7 of the first fragment swapped (last axis)."""
    y = x.copy()
    y[..., 0:4], y[..., 4:8] = x[..., 4:8], x[..., 0:4]
    return y


def emulate(kind, form, inp, defect=None):
    """-> dict(ctx (N L, A 64), dqkv (N L, 3 A 64), lse, delta (N, A, Lp; long), bias_part (N, 3 A 64; l32), guard {name: bool}):
    what the kernels store, float64 of fp32 / 16-bit values; lse and delta start at SENT like the GPU file's buffers.  guard[name]
    is False where the modelled kernel wrote behind an output (the spare-wave defects)."""
    assert form == inp["form"] and (defect is None or defect in DEFECTS), defect
    N, L, A = inp["dims"]
    Lp, HD = pitch(form, L), A * D
    r16 = lambda x: RR.r16(x, kind).astype(F32)
    T_ = lambda x: np.ascontiguousarray(x.transpose(0, 1, 3, 2))
    cl = np.minimum(np.arange(Lp), L - 1)                   # row indices are clamped to L - 1 (:76, :406, :419)
    qh, kh, vh = [heads(inp["qkv"][:, i * HD:(i + 1) * HD], N, L, A).astype(F32)[:, :, cl] for i in range(3)]
    dO = heads(inp["dctx"], N, L, A).astype(F32)[:, :, cl]
    dOc = dO.copy()
    if defect not in ("dO_pad_long", "dO_pad_l32"):
        dO[:, :, L:] = 0                                    # :208, :549, :680
    mask = inp["mask_add"].astype(F32).copy()
    if defect == "unmasked_pad" and L < Lp:
        mask[:, L] = mask[:, L - 1]
    rel = inp["rel"].astype(F32)
    relk = np.ascontiguousarray(rel.transpose(0, 2, 1)) if defect in ("rel_T_long", "rel_T_l32") else rel     # the key-lane view
    score = lambda kk, mk, rl: ((qh @ T_(kk)) * F32(0.125) + mk[:, None, None, :]) + rl[None]
    guard = dict(ctx=True, dqkv=True, lse=True, delta=True, bias_part=True)
    out = dict(guard=guard)
    if form == "l32":
        s = score(kh, mask, rel)
        mx = s.max(-1, keepdims=True)
        e = _expf(s - mx)
        sm = e.sum(-1, keepdims=True, dtype=F32)
        P = e * (F32(1) / sm)
        P16 = r16(P)
        ctx = r16((_swap48(P16) if defect == "perm" else P16) @ vh)
        dP = dO @ T_(vh)
        dsum = (P * dP).sum(-1, keepdims=True, dtype=F32)
        dq = r16((r16(P * (dP - dsum)) @ kh) * F32(0.125))
        lse = mx + _logf(sm)
        pn = _expf(score(kh, mask, relk) - lse)
        dv = r16(T_(r16(pn)) @ dO)
        dk = r16((T_(r16(pn * (dP - dsum))) @ qh) * F32(1.0 if defect == "dk_no_scale" else 0.125))
        bias = np.concatenate([rows(x).reshape(N, Lp, HD).sum(1, dtype=F32) for x in (dq, dk, dv)], 1).astype(F64)
        if defect == "bias_row":
            bias = np.roll(bias, 1, axis=0)
        out["bias_part"] = bias
        if defect == "spare_l32" and (N * A) % 4:           # pairs N A .. 4 ceil(N A / 4) - 1 store their copy at rows >= N L
            guard["ctx"] = guard["dqkv"] = False
    else:
        nt = Lp // 32
        m_run = np.full((N, A, Lp), NEG_BIG, F32)
        l_run = np.zeros((N, A, Lp), F32)
        o = np.zeros((N, A, Lp, D), F32)
        alpha_prev = np.ones((N, A, Lp), F32)
        for kt in range(nt):
            t = slice(32 * kt, 32 * kt + 32)
            s = score(kh[:, :, t], mask[:, t], rel[:, :, t])
            m_new = np.maximum(m_run, s.max(-1))
            alpha = _expf(m_run - m_new)
            p = _expf(s - m_new[..., None])
            l_run = l_run * (alpha_prev if defect == "stale_l" else alpha) + p.sum(-1, dtype=F32)
            alpha_prev, m_run = alpha, m_new
            if not (defect == "skip_rescale" and kt == nt - 1):
                o = o * alpha[..., None]
            p16 = r16(p)
            o = o + (_swap48(p16) if defect == "perm_long" and kt == 0 else p16) @ vh[:, :, t]
        ctx = r16(o * (F32(1) / l_run)[..., None])
        lse = m_run + _logf(l_run)                           # rows L .. Lp too: query L - 1 under the rel row of its own index
        ctx_in = ctx[:, :, cl]
        delta = (dOc * ctx_in).sum(-1, dtype=F32)
        delta[:, :, L:] = 0                                  # :555
        p = _expf(score(kh, mask, rel) - lse[..., None])
        dP = dO @ T_(vh)
        dq = r16((r16(p * (dP - delta[..., None])) @ kh) * F32(0.125))
        pn = _expf(score(kh, mask, relk) - lse[..., None])
        dv = r16(T_(r16(pn)) @ dO)
        dk = r16((T_(r16(pn * (dP - delta[..., None]))) @ qh) * F32(1.0 if defect == "dk_no_scale" else 0.125))
        out["lse"], out["delta"] = lse.astype(F64), delta.astype(F64)
        if defect == "spare_long" and nt % 4:               # waves nt .. 4 ceil(nt / 4) - 1 store at their own tile index
            guard["lse"] = guard["delta"] = guard["ctx"] = guard["dqkv"] = False
    out["ctx"] = rows(ctx[:, :, :L]).astype(F64)
    out["dqkv"] = np.concatenate([rows(x[:, :, :L]) for x in (dq, dk, dv)], 1).astype(F64)
    return out


# ------------------------------------------------------------------------------------------------ the checks
def split(got, inp):
    """The stored layouts -> the reference's: {ctx, dq, dk, dv (N, A, L, 64), lse, delta (N, A, L)}."""
    N, L, A = inp["dims"]
    HD = A * D
    o = dict(ctx=heads(got["ctx"], N, L, A))
    if "dqkv" in got:
        for i, n in enumerate(("dq", "dk", "dv")):
            o[n] = heads(got["dqkv"][:, i * HD:(i + 1) * HD], N, L, A)
    for n in ("lse", "delta"):
        if n in got:
            o[n] = got[n][:, :, :L]
    return o


def failures(kind, inp, r, b, got, emu=None, tag="", log=print):
    """Every check that does not need the device, on one set of outputs `got` (emulate()'s layout) -> (the names of the failed ones,
    {output: (max |err|, worst err / bound, ||got - ref||_F / ||emu - ref||_F)}).  emu: emulate() of the same inputs."""
    N, L, A = inp["dims"]
    HD = A * D
    bad, stats = [], {}
    for n, ok in got["guard"].items():
        if not ok:
            bad.append("guard:" + n)
    g, e = split(got, inp), (split(emu, inp) if emu is not None else None)
    for n in OUTS:
        if n not in g:
            continue
        err = np.abs(g[n] - r[n])
        ratio = float(np.where(err == 0, 0.0, err / np.maximum(b[n], 1e-300)).max(initial=0.0))
        if not np.isfinite(g[n]).all():
            bad.append("finite:" + n)
        elif not (err <= b[n]).all():
            bad.append("elem:" + n)
        fr = float("nan")
        if e is not None and n in e:
            ng, ne = float(np.linalg.norm(g[n] - r[n])), float(np.linalg.norm(e[n] - r[n]))
            fr = ng / ne if ne > 0 else (0.0 if ng == 0 else float("inf"))
            if not ng <= MARGIN * ne:
                bad.append("frob:" + n)
        stats[n] = (float(err.max(initial=0.0)), ratio, fr)
        log("[attn] %s %s %s: max|err| %.3e, worst err / bound %.3f, Frobenius kernel / model %.3f" % (tag, kind, n, stats[n][0], ratio, fr))
    if "delta" in got and not (got["delta"][:, :, L:] == 0).all():
        bad.append("delta_pad")
    if "lse" in got and not np.isfinite(got["lse"][:, :, L:]).all():
        bad.append("lse_pad")
    if "bias_part" in got:
        # each row n on its own: the float64 column sum of the output's OWN 16-bit rows of sequence n, fixed-order fp32 bound
        d3 = got["dqkv"].reshape(N, L, 3 * HD)
        err = np.abs(got["bias_part"] - d3.sum(1))
        bnd = L * U23 * np.abs(d3).sum(1)
        ratio = float(np.where(err == 0, 0.0, err / np.maximum(bnd, 1e-300)).max(initial=0.0))
        log("[attn] %s %s bias_part rows: max|err| %.3e, worst err / bound %.3f" % (tag, kind, float(err.max(initial=0.0)), ratio))
        stats["bias_part"] = (float(err.max(initial=0.0)), ratio, float("nan"))
        if not (err <= bnd).all():
            bad.append("bias_rows")
    return bad, stats
