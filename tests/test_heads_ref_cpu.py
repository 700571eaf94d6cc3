"""tests/heads_ref.py (the float64 references of tests/test_heads_kernels_gpu.py) against oracle/newsrec_oracle.py under identical
inputs: the oracle is pinned to the reference implementation by the goldens of tests/test_oracle_golden.py, so this ties the new
references to it as well.  The loss part of model_fwd / model_bwd is reached with the news encoder replaced by a table of given
vectors (its forward returns them, its backward records the gradient it is handed).

Bound (the form of tests/test_dropout_ref_cpu.py): the oracle computes in fp32, the references in float64 -> rtol 1e-5, and since
an fp32 sum's rounding error is relative to its terms, not to a result that cancels, every comparison also allows 1e-5 of the
tensor's largest magnitude.  Outputs that are cancelling sums - zero in exact arithmetic - are held absolutely against the size of
their neighbour instead (see near_zero); nothing else is exempted."""
import numpy as np
import pytest

import heads_ref as R
from oracle import newsrec_oracle as O

RTOL = 1e-5
B, U, C, D, Q, NT = 3, 7, 4, 16, 12, 3


def close(got, want, what):
    want = np.asarray(want, np.float64)
    assert np.shape(got) == want.shape, what
    np.testing.assert_allclose(got, want, rtol=RTOL, atol=RTOL * np.abs(want).max(initial=0.0), err_msg=what)


def near_zero(got, want, neighbour, what):
    """A cancelling sum: the fc2 bias gradient is sum_u alpha_u (dw_u - S) = S (1 - sum alpha), zero in exact arithmetic up to the
    1e-8 of the normaliser, so the oracle's fp32 value is rounding noise of terms the size of the fc2 WEIGHT gradient's.  It is held
    absolutely against that neighbour (tests/test_kernels_gpu.py::test_attpool_long_equals_the_one_workgroup_kernels does the
    same for db2_part).  The key-projection bias gradient of the raw-exp attention cancels the same way (sum_j ds_ij =
    r_i (1 - sum_j attn_ij)) and is held against the key-projection weight gradient."""
    lim = RTOL * np.abs(np.asarray(neighbour, np.float64)).max()
    assert np.abs(np.asarray(want, np.float64)).max() <= lim, what + " (float64 reference)"
    assert np.abs(np.asarray(got, np.float64) - want).max() <= lim, what


def rnd(rs, *shape, scale=1.0):
    return (rs.standard_normal(shape) * scale).astype(np.float32)


def user_params(rs, pfx, d=D):
    return {pfx + "pad_doc": rnd(rs, 1, d), pfx + "attn.att_fc1.weight": rnd(rs, Q, d, scale=0.3),
            pfx + "attn.att_fc1.bias": rnd(rs, Q, scale=0.1), pfx + "attn.att_fc2.weight": rnd(rs, 1, Q, scale=0.4),
            pfx + "attn.att_fc2.bias": rnd(rs, 1, scale=0.1)}


def ref_user(P, pfx, vec, hidx, mask, ulm):
    g = lambda k: P[pfx + k]
    hv = R.blend(vec, hidx, mask, g("pad_doc")[0], ulm)
    return hv, R.user_fwd(hv, mask, g("attn.att_fc1.weight"), g("attn.att_fc1.bias"), g("attn.att_fc2.weight")[0],
                          g("attn.att_fc2.bias")[0], ulm)


def masks(rs):
    m = (rs.rand(B, U) > 0.4).astype(np.float32)
    m[0] = 1
    m[1] = 0
    m[1, 2] = 1              # a single one
    return m


@pytest.mark.parametrize("ulm", [False, True])
def test_user_encoder_forward_and_backward(ulm):
    rs = np.random.RandomState(11)
    P = user_params(rs, "p.")
    vec = rnd(rs, 30, D, scale=0.5)
    hidx = rs.randint(0, 30, (B, U))
    mask = masks(rs)
    out, c = O.user_encoder_fwd(P, "p.", vec[hidx], mask, ulm)
    hv, f = ref_user(P, "p.", vec, hidx, mask, ulm)
    close(c["x"], hv, "hv")
    close(c["e"], f["e"], "e")
    close(c["al"], f["a"], "a")
    close(c["den"][:, 0], f["den"], "den")
    close(c["w"], f["alpha"], "alpha")
    close(out, f["user"], "user")
    duser = rnd(rs, B, D)
    dnews, G = O.user_encoder_bwd(P, "p.", duser, c)
    b = R.user_bwd(hv, mask, P["p.attn.att_fc1.weight"], P["p.attn.att_fc2.weight"][0], f, duser, ulm)
    close(dnews, b["dslot"], "dslot")
    close(G["p.attn.att_fc1.weight"], b["dW1"], "dW1")
    close(G["p.attn.att_fc1.bias"], b["part_b1"].sum(0), "db1")
    close(G["p.attn.att_fc2.weight"][0], b["part_w2"].sum(0), "dw2")
    close(G["p.pad_doc"][0], b["part_pad"].sum(0), "dpad")
    near_zero(G["p.attn.att_fc2.bias"], b["part_b2"].sum(0), b["part_w2"].sum(0), "db2")
    # the scatter into the row table: a row named by several slots gets their sum
    want = np.zeros((30, D))
    for k, r in enumerate(hidx.reshape(-1)):
        want[r] += b["dslot"].reshape(-1, D)[k]
    dvec, mag = R.scatter(hidx, b["dslot"], 30)
    close(dvec, want, "scatter")
    assert (mag >= np.abs(dvec) - 1e-12).all()


@pytest.mark.parametrize("use_mask", [False, True])
@pytest.mark.parametrize("nh", [1, 3])
def test_nrms_self_attention_forward_and_backward(nh, use_mask):
    rs = np.random.RandomState(5 + nh)
    Dh = nh * 16
    x = rnd(rs, B, U, D, scale=0.7)
    W = [rnd(rs, Dh, D, scale=2.0 / np.sqrt(D)) for _ in range(3)]
    bs = [rnd(rs, Dh, scale=0.1) for _ in range(3)]
    mask = masks(rs)
    out, c = O.mhsa_fwd(x, W[0], bs[0], W[1], bs[1], W[2], bs[2], nh, mask if use_mask else None)
    qkv = np.concatenate([R.f64(x) @ R.f64(W[i]).T + R.f64(bs[i]) for i in range(3)], -1)
    f = R.nrms_fwd(qkv, mask, use_mask, nh)
    close(c["sc"], f["sc"], "sc")
    close(c["den"], f["den"], "den")
    close(c["attn"], f["attn"], "attn")
    close(out, f["ctx"], "ctx")
    dctx = rnd(rs, B, U, Dh)
    dx, G = O.mhsa_bwd(dctx, c, W[0], W[1], W[2])
    dqkv = R.nrms_bwd(f, dctx).reshape(B * U, 3 * Dh)
    x2 = R.f64(x).reshape(B * U, D)
    for i, n in enumerate(("W_Q", "W_K", "W_V")):
        blk = dqkv[:, i * Dh:(i + 1) * Dh]
        close(G[n + ".weight"], blk.T @ x2, n + ".weight")
        if n == "W_K":
            near_zero(G[n + ".bias"], blk.sum(0), blk.T @ x2, n + ".bias")
        else:
            close(G[n + ".bias"], blk.sum(0), n + ".bias")
    close(dx.reshape(B * U, D), dqkv @ np.concatenate([R.f64(w) for w in W], 0), "dx")


@pytest.mark.parametrize("ulm", [False, True])
@pytest.mark.parametrize("nt,tau", [(NT, 2.0), (1, 0.5), (0, 1.0)])
def test_loss_part_of_model_fwd_and_bwd(monkeypatch, nt, tau, ulm):
    rs = np.random.RandomState(3 + nt)
    P = user_params(rs, "student.user_encoder.")
    for i in range(nt):
        P.update(user_params(rs, "teachers.%d." % i))
        P["transform_matrix.%d.weight" % i], P["transform_matrix.%d.bias" % i] = rnd(rs, D, D, scale=0.3), rnd(rs, D, scale=0.1)
    vec = rnd(rs, B * (U + C), D, scale=0.5)           # what the news encoder returns: history rows, then candidate rows
    th = [rnd(rs, B, U, D, scale=0.5) for _ in range(nt)]
    tc = [rnd(rs, B, C, D, scale=0.5) for _ in range(nt)]
    mask, label = masks(rs), rs.randint(0, C, B)
    coef = 0.3
    cfg = dict(n_layers=1, heads=1, trainable_layers=[0], user_log_mask=ulm, temperature=tau, coef=coef)
    got_dvec = []
    monkeypatch.setattr(O, "news_encoder_fwd", lambda *a, **k: (vec, None))
    monkeypatch.setattr(O, "news_encoder_bwd", lambda P_, dvec, *a, **k: (got_dvec.append(dvec), {})[1])
    out = O.model_fwd(P, cfg, np.zeros((B, U, 2), np.int64), mask, np.zeros((B, C, 2), np.int64), label, th, tc)
    G = O.model_bwd(P, cfg, out)

    hidx, cidx = np.arange(B * U).reshape(B, U), B * U + np.arange(B * C).reshape(B, C)
    sp = "student.user_encoder."
    hv, f = ref_user(P, sp, vec, hidx, mask, ulm)
    score = R.score_fwd(vec, cidx, f["user"])
    close(out["user"], f["user"], "user")
    close(out["student_score"], score, "score")
    # teachers: user encoder on the teacher's own history rows, the score, the projected rows [news | user]
    t_scores, projs = [], []
    for i in range(nt):
        _, ft = ref_user(P, "teachers.%d." % i, th[i].reshape(B * U, D), hidx, mask, ulm)
        t_scores.append(np.einsum("bcd,bd->bc", R.f64(tc[i]), ft["user"]))
        W, b = R.f64(P["transform_matrix.%d.weight" % i]), R.f64(P["transform_matrix.%d.bias" % i])
        rows = np.concatenate([R.f64(th[i]).reshape(B * U, D), R.f64(tc[i]).reshape(B * C, D), ft["user"]], 0)
        projs.append((rows, rows @ W.T + b))
    ks = R.kd_score_loss(score, np.stack(t_scores) if nt else None, label, tau, coef)
    close(out["target_loss"], ks["target"], "target")
    close(O.cross_entropy_rows(score.astype(np.float32), label).mean(), ks["target"], "cross_entropy_rows")
    close(out["distill_loss"], ks["distill"], "distill")
    close(out["teacher_weights"], ks["tw"], "tw")
    S = np.concatenate([R.f64(vec), f["user"]], 0)
    nn = B * (U + C)
    dS, dP, emb = np.zeros_like(S), None, 0.0
    if nt:
        emb, dS, dP = R.kd_embed_loss(S, np.stack([p for _, p in projs]), ks["tw"], B, U, C)
    close(out["emb_loss"], emb, "emb")
    close(out["total_loss"], ks["distill"] + coef * ks["target"] + emb, "total")
    # backward: what reaches the news encoder, the user encoder's parameters, the projections
    dcand, duser = R.score_bwd(vec, cidx, f["user"], ks["dscore"])
    b = R.user_bwd(hv, mask, P[sp + "attn.att_fc1.weight"], P[sp + "attn.att_fc2.weight"][0], f, duser + dS[nn:], ulm)
    dvec = dS[:nn] + np.concatenate([b["dslot"].reshape(B * U, D), dcand.reshape(B * C, D)], 0)
    close(got_dvec[0], dvec, "dvec")
    close(G[sp + "attn.att_fc1.weight"], b["dW1"], "dW1")
    close(G[sp + "attn.att_fc1.bias"], b["part_b1"].sum(0), "db1")
    close(G[sp + "attn.att_fc2.weight"][0], b["part_w2"].sum(0), "dw2")
    close(G[sp + "pad_doc"][0], b["part_pad"].sum(0), "dpad")
    near_zero(G[sp + "attn.att_fc2.bias"], b["part_b2"].sum(0), b["part_w2"].sum(0), "db2")
    for i in range(nt):
        close(G["transform_matrix.%d.weight" % i], dP[i].T @ projs[i][0], "transform %d weight" % i)
        close(G["transform_matrix.%d.bias" % i], dP[i].sum(0), "transform %d bias" % i)


def test_kd_embed_loss_stage1_layout_is_the_same_formula_with_no_history_rows():
    """U = 0: [B C title rows | B body rows]; against the U > 0 layout with the history rows dropped and the row weight 1 / C."""
    rs = np.random.RandomState(2)
    S, P, tw = rnd(rs, B * (C + 1), D), rnd(rs, 2, B * (C + 1), D), O.softmax(rnd(rs, B, 2))
    loss, dS, dP = R.kd_embed_loss(S, P, tw, B, 0, C)
    ne = np.stack([((S[:B * C] - P[i][:B * C]).astype(np.float64) ** 2).mean(-1).reshape(B, C).mean(-1) for i in range(2)], -1)
    ue = np.stack([((S[B * C:] - P[i][B * C:]).astype(np.float64) ** 2).mean(-1) for i in range(2)], -1)
    close(loss, (ne * tw).sum(-1).mean() + (ue * tw).sum(-1).mean(), "loss")
    eps = 1e-6
    Sp = S.astype(np.float64).copy()
    Sp[5, 3] += eps
    close((R.kd_embed_loss(Sp, P, tw, B, 0, C)[0] - loss) / eps, dS[5, 3], "dS by finite difference")
    assert np.array_equal(dS, -dP.sum(0))


@pytest.mark.parametrize("ams", [True, False])
def test_adam_step(ams):
    """O.amsgrad_step is AMSGrad; plain Adam is the same update with the running maximum forgotten before every step."""
    rs = np.random.RandomState(4)
    n = 257
    p = rnd(rs, n)
    m, v, vm = np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros(n, np.float32)
    rp, rm, rv, rvm = R.f64(p), R.f64(m), R.f64(v), (R.f64(vm) if ams else None)
    for step in range(1, 6):
        g = rnd(rs, n)
        if not ams:
            vm[:] = 0
        O.amsgrad_step(p, g, m, v, vm, step, 1e-2)
        rp, rm, rv, rvm = R.adam_step(rp, g, rm, rv, rvm, step, 1e-2)
        close(p, rp, "p"), close(m, rm, "m"), close(v, rv, "v")
        if ams:
            close(vm, rvm, "vmax")
    # grad_scale multiplies the gradient first
    a = R.adam_step(rp, 0.125 * R.f64(g), rm, rv, rvm, 6, 1e-2)
    b_ = R.adam_step(rp, g, rm, rv, rvm, 6, 1e-2, grad_scale=0.125)
    assert all(np.array_equal(x, y) for x, y in zip(a[:3], b_[:3]))


def test_segment_sum_reduce_desc_and_blend_are_the_plain_sums():
    rs = np.random.RandomState(6)
    src = rnd(rs, 40, 8)
    order = rs.permutation(40)[:25]
    seg = np.array([0, 0, 3, 4, 20, 25, 25])
    out, mag = R.segment_sum(src, order, seg)
    want = np.zeros((6, 8))
    np.add.at(want, np.repeat(np.arange(6), np.diff(seg)), src[order].astype(np.float64))
    close(out, want, "segment_sum")
    assert (out[0] == 0).all() and (out[5] == 0).all() and (mag >= np.abs(out) - 1e-12).all()
    flat = rnd(rs, 200)
    got, mag = R.reduce_desc(flat[3:], 5, 9, 7, dst0=np.ones(7), scale=0.5)
    close(got, 1.0 + 0.5 * sum(flat[3 + r * 9:3 + r * 9 + 7].astype(np.float64) for r in range(5)), "reduce_desc")
    vec, pad = rnd(rs, 10, 4), rnd(rs, 4)
    hidx, mask = np.array([[1, 1, 9]]), np.array([[1.0, 0.0, 0.5]], np.float32)
    hv = R.blend(vec, hidx, mask, pad, False)
    close(hv[0], np.stack([vec[1], pad, 0.5 * vec[9].astype(np.float64) + 0.5 * pad]), "blend")
    assert np.array_equal(R.blend(vec, hidx, mask, pad, True)[0], vec[[1, 1, 9]].astype(np.float64))
