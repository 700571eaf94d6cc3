"""tests/rows_ref.py (the float64 references and bounds of tests/test_rows_kernels_gpu.py) without a GPU:

  * every restatement against oracle/newsrec_oracle.py under identical inputs on small shapes (the oracle is pinned to the reference
    implementation by tests/test_oracle_golden.py): rtol 1e-5 plus 1e-5 of the tensor's largest magnitude, the form of
    tests/test_heads_ref_cpu.py;
  * every bound on every input set the GPU file uses: the fp32 oracle (or, where the oracle has no such function, the same
    formula in numpy float32), rounded once to the 16-bit type by torch on the CPU, has to pass the bound the kernel is held to -
    which shows that a correct fp32 implementation can meet it.  A bound that fails here has a wrong derivation;
  * no bound looser than the flat tolerance tests/test_kernels_gpu.py holds the same output to, element by element, on every
    input set - with the exceptions LOOSER names case by case, each of which is asserted to BE looser, so that the list cannot
    outlive its reasons (den has no tolerance there: that file never compares it);
  * the rel-pos cases put every bucket edge, on both signs, into at least one table."""
import numpy as np
import pytest

import rows_ref as R
from oracle import newsrec_oracle as O

RTOL = 1e-5
F32 = np.float32
FLAT16 = {"bf16": 1e-2, "f16": 1.5e-3}         # tests/test_kernels_gpu.py::test_layernorm_fwd_bwd, rtol = atol


def close(got, want, what):
    want = np.asarray(want, np.float64)
    assert np.shape(got) == want.shape, what
    np.testing.assert_allclose(got, want, rtol=RTOL, atol=RTOL * np.abs(want).max(initial=0.0), err_msg=what)


def within(what, got, ref, bound):
    err = np.abs(np.asarray(got, np.float64) - ref)
    assert np.isfinite(err).all() and (err <= bound).all(), \
        "%s: %d of %d over the bound, worst err / bound %.3f" % (what, int((err > bound).sum()), err.size, float((err / np.maximum(bound, 1e-300)).max()))


# Where a bound IS looser than today's flat tolerance, and why.  Everything not named here is asserted to be no looser.
LOOSER = {
    # rtol 1e-5, atol 1e-6 of test_cls_and_mean_pooling: a sum of 30 rounded additions has (30 + 1) 2^-23 mean|y| = 3e-6
    "pool_fwd": lambda L, **_: L == 30,
    # rtol 1e-4, atol 1e-6 of test_attpool_fwd_bwd: behind __expf alpha keeps the floor 1e-5 max|alpha| of the fp32 head kernels,
    # which is above 1e-6 as soon as one weight is above 0.1
    "alpha": lambda amax, **_: 1e-5 * amax > 1e-6,
    # rtol 1e-2, atol 1e-2 max|dpre| of test_attpool_fwd_bwd: at L = 1 da = alpha (dw - S) and with it dpre are zero in exact
    # arithmetic, so that tolerance is zero, while dw keeps the bound of its dot product
    "dpre": lambda L, **_: L == 1,
    # rtol 1e-3, atol 1e-4 of test_attpool_fwd_bwd on the three per-sequence sums, summed over the sequences.  dw2_part: the dot
    # product dw = dnv . y has sum|dnv||y| = 0.6 H, so even at the depth of its reduction (19 at H = 768) its bound, 1e-3, is ten
    # times that atol where the reference cancels; only H = 4 stays under it
    "dw2_part": lambda H, **_: H > 4,
    # db2_part: zero in exact arithmetic, held to 2e-4 max|dw2_part| per sequence as the chunked kernels are against the
    # one-workgroup ones; under 1e-4 only where dw2_part is small (L = 1: zero; H = 4 at L = 129)
    "db2_part": lambda L, H, **_: not (L == 1 or (L, H) == (129, 4)),
    # db1_part: L 2^-23 sum|dpre| crosses 1e-4 around L = 64 (at 63 and 64 by 5 .. 10 %, at 65 just not) and stays above from 127 on
    "db1_part": lambda L, H, **_: (L in (63, 64) or L >= 127) and H > 4,
    # rtol 1e-4, atol 1e-3 of test_colsum_and_reduce (M = 1234): a 128-deep chain on sum|x| = 26000
    "colsum": lambda M, **_: M == 32768 + 5,
    # rtol = atol = 1e-3 (dgamma, dbeta), rtol 1e-4, atol 1e-3 (dxsum) of test_layernorm_fwd_bwd (M = 5, 257): depth 33 on 26000
    "ln_sums": lambda M, **_: M == 32777,
}


def tighter(what, bound, ref, rtol, atol, rule=None, **case):
    flat = atol + rtol * np.abs(ref)
    ok = bool((bound <= flat).all())
    if rule is not None and LOOSER[rule](**case):
        assert not ok, "%s: named as looser than the flat tolerance, but is not" % what
        return
    assert ok, "%s: bound looser than the flat tolerance, worst bound / flat %.3f" % (what, float((bound / flat).max()))


# ------------------------------------------------------------------------------------------------ ties to the oracle
def test_layernorm_restatements_against_the_oracle():
    c = R.ln_case(9, 256, "f16", True)
    x, dy = c["x"].astype(F32), c["dy"].astype(F32)
    y, (xh, rstd) = O.layer_norm_fwd(x, c["g"], c["b"], R.EPS)
    f = R.ln_fwd(x, c["g"], c["b"])
    close(y, f["y"], "y")
    close(rstd[:, 0], f["rstd"], "rstd")
    dx, dg, db = O.layer_norm_bwd(dy, (xh, rstd), c["g"])
    b = R.ln_bwd(dy, x, f["mean"], f["rstd"], c["g"], "f16")
    close(dx, b["dx"], "dx")
    close(dg, b["dgamma"], "dgamma")
    close(db, b["dbeta"], "dbeta")
    assert np.array_equal(b["dxsum"], R.r16(b["dx"], "f16").sum(0))
    m = (np.random.RandomState(0).rand(9, 256) > 0.1) / 0.9
    bm = R.ln_bwd(dy, x, f["mean"], f["rstd"], c["g"], "f16", mask=m)
    assert np.array_equal(bm["dx"], b["dx"]) and np.array_equal(bm["dxm"], b["dx"] * m)
    assert np.array_equal(bm["dxsum"], R.r16(b["dx"] * m, "f16").sum(0))


def _embed_params(c):
    return {O.BERT + "embeddings.word_embeddings.weight": c["word"], O.BERT + "embeddings.position_embeddings.weight": c["pos"],
            O.BERT + "embeddings.token_type_embeddings.weight": np.stack([c["type0"], c["type0"] + 1]),
            O.BERT + "embeddings.LayerNorm.weight": c["g"], O.BERT + "embeddings.LayerNorm.bias": c["b"]}


def test_embedding_restatement_against_the_oracle():
    c = R.embed_case(3, 7, 256)
    y = O.embeddings_fwd(_embed_params(c), c["ids"])
    close(y.reshape(21, 256), R.embed_ln(c["ids"], c["word"], c["pos"], c["type0"], c["g"], c["b"])["y"], "embed y")
    assert np.array_equal(R.mask_add(np.array([[1, 0]])), np.array([[0.0, -10000.0]], F32))


def _attpool_oracle(c):
    """O.att_pool_fwd from its second line on, on the case's e (the case holds e = tanh(fc1 y) itself, no fc1): -> nv and the cache
    O.att_pool_bwd reads."""
    y = c["y"].astype(F32)
    b2 = np.array([c["b2"]], F32)
    al = np.exp(O.linear(c["e"], c["w2"][None], b2))[..., 0].astype(F32)
    den = al.sum(1, keepdims=True) + F32(1e-8)
    w = (al / den).astype(F32)
    return (w[..., None] * y).sum(1).astype(F32), dict(x=y, e=c["e"], al=al, den=den, w=w, mask=None)


def test_attention_pooling_restatements_against_the_oracle():
    c = R.attpool_case(5, 260, 64, "f16")
    y = c["y"].astype(F32)
    # forward: the oracle's own function on a case whose e it computes itself
    w1, b1 = (0.05 * np.random.RandomState(1).standard_normal((64, 260))).astype(F32), np.zeros(64, F32)
    out, cache = O.att_pool_fwd(y, w1, b1, c["w2"][None], np.array([c["b2"]], F32))
    f = R.attpool_fwd(y, cache["e"], c["w2"], c["b2"])
    close(out, f["nv"], "nv")
    close(cache["w"], f["alpha"], "alpha")
    close(cache["den"][:, 0], f["den"], "den")
    # backward: dx = dy_direct + dpre W1, g_b1 = sum dpre, g_w2 = sum_n dw2_part, g_b2 = sum_n db2_part (a cancelling sum)
    dx, g1, gb1, g2, gb2 = O.att_pool_bwd(c["dnv"], cache, w1, c["w2"][None])
    b = R.attpool_bwd(y, cache["e"], c["w2"], cache["w"], c["dnv"], "f16")
    close(dx, b["dy_direct"] + b["dpre"] @ w1.astype(np.float64), "dx")
    close(gb1, b["dpre"].sum((0, 1)), "g_b1")
    close(g2[0], b["dw2_part"].sum(0), "g_w2")
    close(g1, np.einsum("nlq,nlh->qh", b["dpre"], y.astype(np.float64)), "g_w1")
    lim = RTOL * np.abs(b["dw2_part"]).max()
    assert abs(b["db2_part"].sum()) <= lim and abs(float(gb2[0]) - b["db2_part"].sum()) <= lim
    assert np.array_equal(b["db1_part"], R.r16(b["dpre"], "f16").sum(1))


def test_pool_and_colsum_restatements():
    y, dnv = R.pool_case(5, 30, 256, "bf16")
    close(y.astype(F32).mean(1), R.pool_fwd(y, 1)[0], "mean pooling")
    assert np.array_equal(R.pool_fwd(y, 0)[0], y[:, 0])
    dy, _ = R.pool_bwd(dnv, 30, 1)
    close(np.repeat(dnv[:, None] / F32(30), 30, 1), dy, "mean pooling backward")
    dy, _ = R.pool_bwd(dnv, 30, 0)
    assert np.array_equal(dy[:, 0], dnv) and (dy[:, 1:] == 0).all()
    x, o = R.colsum_case(65, 260, "bf16")
    close(o[0] + x[0].astype(F32).sum(0), R.colsum(x[0], o[0])[0], "colsum")


# ------------------------------------------------------------------------------------------------ the bounds without the kernel
def _ln_fwd_f32(x, g, b):
    x = x.astype(F32)
    y, (xh, rstd) = O.layer_norm_fwd(x, g, b, R.EPS)
    return y, x.mean(-1, dtype=F32), rstd[:, 0]


def _sum_f32(x):
    """Column sums in float32, rows added one after the other."""
    return np.asarray(x, F32).sum(0, dtype=F32)


def _ln_cases():
    for H in R.LN_H:
        for M in R.LN_M:
            yield M, H
    yield R.LN_TALL[-1], 256


@pytest.mark.parametrize("kind", R.KINDS)
def test_layernorm_bounds_hold_for_the_fp32_oracle(kind):
    for M, H in _ln_cases():
        tag = "M%d H%d %s" % (M, H, kind)
        if M <= 65:                                        # forward: rows of all four kinds
            c = R.ln_case(M, H, kind, False)
            f = R.ln_fwd(c["x"], c["g"], c["b"])
            y, mean, rstd = _ln_fwd_f32(c["x"], c["g"], c["b"])
            within("y " + tag, R.r16(y, kind), f["y"], R.out16(f["y"], kind, f["fp_y"]))
            within("mean " + tag, mean, f["mean"], f["b_mean"])
            within("rstd " + tag, rstd, f["rstd"], f["b_rstd"])
            tighter("y " + tag, R.out16(f["y"], kind, f["fp_y"]), f["y"], FLAT16[kind], FLAT16[kind])
            const = c["rk"] == 3
            assert np.array_equal(R.r16(y, kind)[const], np.broadcast_to(R.r16(c["b"], kind), (int(const.sum()), H)))
            assert np.array_equal(mean[const], c["x"][const, 0])
        c = R.ln_case(M, H, kind, True)
        f = R.ln_fwd(c["x"], c["g"], c["b"])
        st = R.ln_stats32(f)
        b = R.ln_bwd(c["dy"], c["x"], st[:, 0], st[:, 1], c["g"], kind)
        x, dy = c["x"].astype(F32), c["dy"].astype(F32)
        xh = (x - st[:, :1]) * st[:, 1:]
        dx, dg, db = O.layer_norm_bwd(dy, (xh, st[:, 1:]), c["g"])
        within("dx " + tag, R.r16(dx, kind), b["dx"], R.out16(b["dx"], kind, b["fp_dx"]))
        within("dgamma " + tag, dg, b["dgamma"], b["b_dgamma"])
        within("dbeta " + tag, db, b["dbeta"], b["b_dbeta"])
        dx16 = R.r16(dx, kind)
        own = R.colsum_bound(dx16, b["count"])               # against the sums of the SAME rounded values, as the GPU file does
        within("dxsum (own) " + tag, _sum_f32(dx16), dx16.sum(0), own)
        within("dxsum " + tag, _sum_f32(dx16), b["dxsum"], b["b_dxsum"])
        tighter("dx " + tag, R.out16(b["dx"], kind, b["fp_dx"]), b["dx"], FLAT16[kind], FLAT16[kind])
        tighter("dgamma " + tag, b["b_dgamma"], b["dgamma"], 1e-3, 1e-3, "ln_sums", M=M)
        tighter("dbeta " + tag, b["b_dbeta"], b["dbeta"], 1e-3, 1e-3, "ln_sums", M=M)
        tighter("dxsum " + tag, own, dx16.sum(0), 1e-4, 1e-3, "ln_sums", M=M)


@pytest.mark.parametrize("kind", R.KINDS)
def test_layernorm_masked_output_bound_holds_for_the_fp32_oracle(kind):
    from oracle import dropout_oracle as DO
    for H, M in R.LN_DO:
        c = R.ln_case(M, H, kind, True)
        st = R.ln_stats32(R.ln_fwd(c["x"], c["g"], c["b"]))
        m = DO.rows_mask(0.1, 1234, DO.site_id(DO.KIND_FFN_OUT, 1), 3, M, H)
        b = R.ln_bwd(c["dy"], c["x"], st[:, 0], st[:, 1], c["g"], kind, mask=m)
        x, dy = c["x"].astype(F32), c["dy"].astype(F32)
        dx, _, _ = O.layer_norm_bwd(dy, ((x - st[:, :1]) * st[:, 1:], st[:, 1:]), c["g"])
        dxm16 = R.r16(dx * m, kind)
        within("dxm M%d H%d" % (M, H), dxm16, b["dxm"], R.out16(b["dxm"], kind, b["fp_dxm"]))
        within("dxsum (own) M%d H%d" % (M, H), _sum_f32(dxm16), dxm16.sum(0), R.colsum_bound(dxm16, b["count"]))
        within("dxsum M%d H%d" % (M, H), _sum_f32(dxm16), b["dxsum"], b["b_dxsum"])
        assert (b["dxm"][m == 0] == 0).all() and (m == 0).any()


@pytest.mark.parametrize("kind", R.KINDS)
def test_embedding_bound_holds_for_the_fp32_oracle(kind):
    for H in R.LN_H:
        for N, L in R.EMBED_NL:
            c = R.embed_case(N, L, H)
            f = R.embed_ln(c["ids"], c["word"], c["pos"], c["type0"], c["g"], c["b"])
            y = O.embeddings_fwd(_embed_params(c), c["ids"]).reshape(N * L, H)
            bound = R.out16(f["y"], kind, f["fp_y"])
            within("embed N%d L%d H%d" % (N, L, H), R.r16(y, kind), f["y"], bound)
            tighter("embed N%d L%d H%d" % (N, L, H), bound, f["y"], 1e-2, 1e-2)
            assert (c["ids"].min() == 0 or N * L == 1) and c["ids"].max() == R.VOCAB - 1 and (N < 2 or c["mask"][N - 1].sum() == 0)
            assert c["nidx"].max() == len(c["table"]) - 1 and (N < 3 or len(set(c["nidx"].tolist())) < N)


@pytest.mark.parametrize("kind", R.KINDS)
def test_pooling_and_colsum_bounds_hold_in_float32(kind):
    for H in R.POOL_H:
        for L in R.POOL_L:
            for n in R.POOL_N:
                y, dnv = R.pool_case(n, L, H, kind)
                ref, bound = R.pool_fwd(y, 1)
                acc = np.zeros((n, H), F32)
                for i in range(L):
                    acc += y[:, i].astype(F32)
                within("pool mean", acc * (F32(1.0) / F32(L)), ref, bound)
                tighter("pool mean L%d H%d" % (L, H), bound, ref, 1e-5, 1e-6, "pool_fwd", L=L)
                dy, fp = R.pool_bwd(dnv, L, 1)
                got = R.r16(np.repeat((dnv * (F32(1.0) / F32(L)))[:, None], L, 1), kind)
                within("pool mean bwd", got, dy, R.out16(dy, kind, fp))
                tighter("pool mean bwd", R.out16(dy, kind, fp), dy, 1e-2, 1e-3)
                dy, fp = R.pool_bwd(dnv, L, 0)
                within("pool cls bwd", R.r16(dy, kind), dy, R.out16(dy, kind, fp))
    for k in (kind, "f32"):
        for M, N in R.COLSUM_SHAPES:
            x, o = R.colsum_case(M, N, k)
            for out0 in (None, o[0]):
                ref, bound = R.colsum(x[0], out0)
                s = np.zeros(N, F32) if out0 is None else out0.copy()
                got = x[0].astype(F32).sum(0, dtype=F32) + s
                within("colsum M%d N%d" % (M, N), got, ref, bound)
                tighter("colsum M%d N%d" % (M, N), bound, ref, 1e-4, 1e-3, "colsum", M=M)
        for batch, M, N in R.COLSUM_BATCHED:
            x, o = R.colsum_case(M, N, k, batch)
            for out0 in (None, o):
                ref, bound = R.colsum(x, out0)
                got = np.stack([_sum_f32(x[z]) for z in range(batch)]) + (F32(0) if out0 is None else out0)
                within("colsum_batched b%d M%d N%d" % (batch, M, N), got, ref, bound)
                tighter("colsum_batched b%d M%d N%d" % (batch, M, N), bound, ref, 1e-4, 1e-3)


def _attpool_f32(c, kind):
    """The pooling forward through the oracle (its cache overwritten with the case's e) and the backward's pieces in float32, in
    the oracle's formulation (att_pool_bwd: dal = (dw - sum dw w) / den, da = dal al)."""
    nv, cache = _attpool_oracle(c)
    y, w, e, w2 = c["y"].astype(F32), cache["w"], c["e"], c["w2"]
    dw = (y * c["dnv"][:, None, :]).sum(-1)
    da = (dw - (dw * w).sum(1, keepdims=True)) / cache["den"] * cache["al"]
    dpre = (da[..., None] * w2[None, None, :] * (F32(1.0) - e * e)).astype(F32)
    return nv, cache, dict(dy_direct=R.r16(w[..., None] * c["dnv"][:, None, :], kind), dpre=R.r16(dpre, kind),
                           dw2_part=(da[..., None] * e).sum(1), db2_part=da.sum(1))


@pytest.mark.parametrize("kind", R.KINDS)
def test_attention_pooling_bounds_hold_for_the_fp32_oracle(kind):
    for L, H, Q, _, _ in sorted(set(R.attpool_cases(False) + R.attpool_cases(True))):
        tag = "L%d H%d Q%d %s" % (L, H, Q, kind)
        c = R.attpool_case(L, H, Q, kind)
        f = R.attpool_fwd(c["y"], c["e"], c["w2"], c["b2"])
        nv, cache, g = _attpool_f32(c, kind)
        for name, got in (("nv", nv), ("alpha", cache["w"]), ("den", cache["den"][:, 0])):
            within(name + " " + tag, got, f[name], R.FWD * np.abs(f[name]) + R.FLOOR * np.abs(f[name]).max())
        b = R.attpool_bwd(c["y"], c["e"], c["w2"], cache["w"], c["dnv"], kind)
        for name in ("dy_direct", "dpre"):
            within(name + " " + tag, g[name], b[name], R.out16(b[name], kind, b["fp_" + name]))
        within("dw2_part " + tag, g["dw2_part"], b["dw2_part"], b["b_dw2_part"])
        within("db2_part " + tag, g["db2_part"], b["db2_part"], R.DB2 * np.abs(b["dw2_part"]).max())
        d16 = g["dpre"]
        within("db1_part (own) " + tag, np.stack([_sum_f32(d) for d in d16]), d16.sum(1), L * R.U23 * np.abs(d16).sum(1))
        within("db1_part " + tag, np.stack([_sum_f32(d) for d in d16]), b["db1_part"], b["b_db1_part"])
        fwd = lambda name: R.FWD * np.abs(f[name]) + R.FLOOR * np.abs(f[name]).max()
        tighter("nv " + tag, fwd("nv"), f["nv"], 1e-4, 1e-4)
        tighter("alpha " + tag, fwd("alpha"), f["alpha"], 1e-4, 1e-6, "alpha", amax=f["alpha"].max())
        # the three per-sequence sums, summed over the sequences as test_attpool_fwd_bwd compares them (rtol 1e-3, atol 1e-4)
        tighter("dw2_part " + tag, b["b_dw2_part"].sum(0), b["dw2_part"].sum(0), 1e-3, 1e-4, "dw2_part", L=L, H=H)
        tighter("db2_part " + tag, len(d16) * R.DB2 * np.abs(b["dw2_part"]).max(), b["db2_part"].sum(), 1e-3, 1e-4, "db2_part", L=L, H=H)
        tighter("db1_part " + tag, (L * R.U23 * np.abs(d16).sum(1)).sum(0), d16.sum((0, 1)), 1e-3, 1e-4, "db1_part", L=L, H=H)
        tighter("dy_direct " + tag, R.out16(b["dy_direct"], kind, b["fp_dy_direct"]), b["dy_direct"], 1e-2, 1e-3)
        tighter("dpre " + tag, R.out16(b["dpre"], kind, b["fp_dpre"]), b["dpre"], 1e-2, 1e-2 * np.abs(b["dpre"]).max(), "dpre", L=L, H=H)


# ------------------------------------------------------------------------------------------------ rel-pos cases, shadow sources
def test_relpos_cases_reach_every_bucket_edge_on_both_signs():
    for a, b in R.RELPOS_EDGES:
        assert O.relative_position_bucket(np.array([a]))[0] != O.relative_position_bucket(np.array([b]))[0]
        for sign in (1, -1):
            hit = []
            for L in R.RELPOS_L:
                pos = np.arange(L)
                rel = pos[None, :] - pos[:, None]
                if (rel == sign * a).any() and (rel == sign * b).any():
                    t = R.relpos_table(np.arange(32, dtype=F32)[None], L)[0]          # weight = bucket number
                    assert set(t[rel == sign * a]) != set(t[rel == sign * b])
                    hit.append(L)
            assert hit, "edge %d/%d, sign %d" % (a, b, sign)
    assert {L - 1 for L in R.RELPOS_L} >= {31, 32, 90, 91}       # an edge distance as the table's largest, and one past it


@pytest.mark.parametrize("kind", R.KINDS)
def test_shadow_sources_hold_ties_of_both_parities_subnormals_and_minus_zero(kind):
    src = R.shadow_source(31, 33, kind, 1)
    bits = R.shadow_cast(src, kind).view(np.uint16).reshape(-1)
    assert bits[0] == 0x8000                                         # -0.0 stays -0.0
    one = 0x3F80 if kind == "bf16" else 0x3C00
    assert bits[1] == one and bits[2] == one + 2                     # ties: down to the even neighbour, up to the even neighbour
    sub = R.r16(src, kind).reshape(-1)
    small = 2.0 ** -126 if kind == "bf16" else 2.0 ** -14
    assert ((np.abs(sub) < small) & (sub != 0)).any()                # a value that lands among the type's subnormals
    if kind == "f16":
        assert np.isinf(sub).sum() == 2 and sub[10] == 65504.0        # 65520 and 70000 round to infinity, 65519 does not
    assert np.array_equal(R.shadow_source(1, 1, kind, 1).view(np.uint32), [[0x80000000]])
