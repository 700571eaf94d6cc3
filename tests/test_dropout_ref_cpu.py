"""tests/dropout_ref.py (the float64 references of tests/test_dropout_kernels_gpu.py) against oracle/newsrec_oracle.py under the same
oracle/dropout_oracle.Dropout, on a tiny layer: the oracle is pinned to the reference implementation by
tests/golden/stage1_cfg4_drop.npz (tests/test_oracle_golden.py), so this ties the new references to it as well.

Bound: the oracle computes in fp32, the helpers in float64 -> rtol 1e-5.  An fp32 sum's rounding error is relative to its terms,
not to a result that cancels, so every comparison also allows 1e-5 of the tensor's largest magnitude."""
import numpy as np
import pytest

import dropout_ref as R
from oracle import dropout_oracle as DO
from oracle import newsrec_oracle as O

N, L, H, A, I, V, LAYER = 3, 11, 64, 4, 256, 50, 1
RTOL = 1e-5


def close(got, want, what):
    want = np.asarray(want, np.float64)
    np.testing.assert_allclose(got, want, rtol=RTOL, atol=RTOL * np.abs(want).max(), err_msg=what)


def _layer_params():
    rs = np.random.RandomState(7)
    r = lambda *s, scale=0.3: (rs.standard_normal(s) * scale).astype(np.float32)
    p = O._lp(LAYER)
    P = {}
    for n in ("query", "key", "value"):
        P[p + "attention.self.%s.weight" % n], P[p + "attention.self.%s.bias" % n] = r(H, H), r(H)
    P[p + "attention.output.dense.weight"], P[p + "attention.output.dense.bias"] = r(H, H, scale=0.15), r(H)
    P[p + "intermediate.dense.weight"], P[p + "intermediate.dense.bias"] = r(I, H, scale=0.15), r(I)
    P[p + "output.dense.weight"], P[p + "output.dense.bias"] = r(H, I, scale=0.1), r(H)
    for n in ("attention.output.LayerNorm", "output.LayerNorm"):
        P[p + n + ".weight"], P[p + n + ".bias"] = 1 + r(H, scale=0.1), r(H, scale=0.1)
    return P, rs


@pytest.fixture(scope="module")
def layer():
    P, rs = _layer_params()
    x = rs.standard_normal((N, L, H)).astype(np.float32)
    mask = (rs.rand(N, L) > 0.3).astype(np.float32)
    mask[0] = 1
    mask[1, 1:] = 0              # one key left.  (No all-pad sequence here: its scores are all -10000 + x, which fp32 resolves to
    #                              ulp(10000) / 2 = 4.9e-4 only, so the fp32 oracle itself is 1e-3 off there; the GPU tests have one.)
    mask_add = ((1.0 - mask) * -10000.0).astype(np.float32)
    rel = O.relpos_bias_table((rs.standard_normal((A, 32)) * 0.5).astype(np.float32), L)
    dy = rs.standard_normal((N, L, H)).astype(np.float32)
    return P, x, mask_add, rel, dy


def _helpers_forward(P, x, mask_add, rel, c):
    """The layer through dropout_ref's helpers, with the masks the oracle's cache holds (None in eval mode)."""
    p = O._lp(LAYER)
    g = lambda k: P[p + k]
    x2 = x.reshape(N * L, H)
    qkv = np.concatenate([R.linear_do(x2, g("attention.self.%s.weight" % n), g("attention.self.%s.bias" % n))
                          for n in ("query", "key", "value")], 1)
    at = R.attn_fwd(qkv, mask_add, rel, N, L, A, m=c["mp"], d=H // A)
    h1 = R.layer_norm(R.linear_do(at["ctx"], g("attention.output.dense.weight"), g("attention.output.dense.bias"), m=c["mo"], res=x2),
                      g("attention.output.LayerNorm.weight"), g("attention.output.LayerNorm.bias"), 1e-12)
    act = R.linear_do(h1, g("intermediate.dense.weight"), g("intermediate.dense.bias"), act=R.gelu)
    y = R.layer_norm(R.linear_do(act, g("output.dense.weight"), g("output.dense.bias"), m=c["mf"], res=h1),
                     g("output.LayerNorm.weight"), g("output.LayerNorm.bias"), 1e-12)
    return at, h1, y


@pytest.mark.parametrize("p_hidden,p_attn", [(0.1, 0.1), (0.5, 0.5), (0.0, 0.3), (0.0, 0.0)])
def test_helpers_equal_the_oracle_layer_forward_and_backward(layer, p_hidden, p_attn):
    P, x, mask_add, rel, dy = layer
    drop = DO.Dropout(p_hidden, p_attn, 0xC0FFEE, 3) if (p_hidden or p_attn) else None
    y_o, c = O.bert_layer_fwd(P, LAYER, x, mask_add, rel, A, drop=drop)
    assert (c["mp"] is not None) == (p_attn > 0) and (c["mo"] is not None) == (p_hidden > 0)
    at, h1, y = _helpers_forward(P, x, mask_add, rel, c)
    close(at["p"], c["pr"], "probabilities (the mask is not in them)")
    close(at["ctx"], c["ctx"].reshape(N * L, H), "ctx")
    close(h1, c["h1"].reshape(N * L, H), "attention-output Linear + dropout + residual -> LayerNorm")
    close(y, y_o.reshape(N * L, H), "layer output")
    # lse against the oracle's scores, restated: log sum exp over every key
    d = H // A
    s = (c["qh"] @ c["kh"].transpose(0, 1, 3, 2)).astype(np.float64) / np.sqrt(d) + mask_add[:, None, None, :] + rel[None]
    close(at["lse"], np.log(np.exp(s - s.max(-1, keepdims=True)).sum(-1)) + s.max(-1), "lse")

    # backward: the oracle's own chain down to dctx (oracle/newsrec_oracle.py bert_layer_bwd), then the helper
    dx_o, G = O.bert_layer_bwd(P, LAYER, dy, c, A)
    p = O._lp(LAYER)
    dypre, _, _ = O.layer_norm_bwd(dy, c["ln2"], P[p + "output.LayerNorm.weight"])
    dres2 = dypre
    if c["mf"] is not None:
        dypre = dypre * c["mf"].reshape(dypre.shape)
    du = (dypre @ P[p + "output.dense.weight"]) * O.gelu_grad(c["u"])
    dh1pre, _, _ = O.layer_norm_bwd((dres2 + du @ P[p + "intermediate.dense.weight"]).astype(np.float32), c["ln1"],
                                    P[p + "attention.output.LayerNorm.weight"])
    dres1 = dh1pre
    if c["mo"] is not None:
        dh1pre = dh1pre * c["mo"].reshape(dh1pre.shape)
    dctx = (dh1pre @ P[p + "attention.output.dense.weight"]).reshape(N * L, H)
    dqkv, _ = R.attn_bwd(at, dctx)
    x2 = x.reshape(N * L, H).astype(np.float64)
    dx = dres1.reshape(N * L, H).astype(np.float64)
    for i, n in enumerate(("query", "key", "value")):
        t = dqkv[:, i * H:(i + 1) * H]
        close(t.T @ x2, G[p + "attention.self.%s.weight" % n], n + " weight gradient")
        if n != "key":          # the key bias is a mathematical no-op: its gradient is rounding noise on both sides
            close(t.sum(0), G[p + "attention.self.%s.bias" % n], n + " bias gradient")
        dx = dx + t @ P[p + "attention.self.%s.weight" % n].astype(np.float64)
    close(dx, dx_o.reshape(N * L, H), "dx")


def test_attention_mask_sits_where_the_oracle_puts_it(layer):
    """A mask with a single zero moves exactly the outputs the oracle moves: row i of ctx and dq, rows j of dk / dv."""
    P, x, mask_add, rel, dy = layer
    rs = np.random.RandomState(1)
    qkv = rs.standard_normal((N * L, 3 * H))
    dctx = rs.standard_normal((N * L, H))
    m = np.ones((N, A, L, L))
    n, a, i, j = 0, 1, 4, 9        # sequence 0 has no padding: P[n, a, i, j] > 0
    m[n, a, i, j] = 0.0
    base, one = R.attn_fwd(qkv, mask_add, rel, N, L, A, d=H // A), R.attn_fwd(qkv, mask_add, rel, N, L, A, m=m, d=H // A)
    d = H // A
    diff = np.abs(one["ctx"] - base["ctx"]).reshape(N, L, A, d).sum(-1) > 0
    want = np.zeros((N, L, A), bool)
    want[n, i, a] = True
    assert np.array_equal(diff, want) and np.array_equal(one["lse"], base["lse"])
    gb, go = R.attn_bwd(base, dctx)[0], R.attn_bwd(one, dctx)[0]
    dv = np.abs(go - gb)[:, 2 * H:].reshape(N, L, A, d).sum(-1) > 0
    want_v = np.zeros((N, L, A), bool)
    want_v[n, j, a] = True
    assert np.array_equal(dv, want_v)
    dq = np.abs(go - gb)[:, :H].reshape(N, L, A, d).sum(-1) > 0
    assert np.array_equal(dq, want)


@pytest.mark.parametrize("pos_pad", [None, 1])
@pytest.mark.parametrize("p_hidden", [0.0, 0.1, 0.5])
def test_embedding_helper_equals_the_oracle(pos_pad, p_hidden):
    rs = np.random.RandomState(11)
    n_seq, Le = 5, 13
    P = {O.BERT + "embeddings.word_embeddings.weight": rs.standard_normal((V, H)).astype(np.float32),
         O.BERT + "embeddings.position_embeddings.weight": rs.standard_normal((Le + 2, H)).astype(np.float32),
         O.BERT + "embeddings.token_type_embeddings.weight": rs.standard_normal((2, H)).astype(np.float32),
         O.BERT + "embeddings.LayerNorm.weight": (1 + 0.1 * rs.standard_normal(H)).astype(np.float32),
         O.BERT + "embeddings.LayerNorm.bias": (0.1 * rs.standard_normal(H)).astype(np.float32)}
    ids = rs.randint(2, V, (n_seq, Le))
    ids[0, 7:] = 1
    ids[1, :] = 1                # an all-pad row (RoBERTa's padding_idx)
    ids[2, 3] = 1                # a pad inside a row
    drop = DO.Dropout(p_hidden, 0.0, 99, 2) if p_hidden else None
    want = O.embeddings_fwd(P, ids, drop=drop, pos_pad=pos_pad).reshape(n_seq * Le, H)
    m = DO.rows_mask(p_hidden, 99, DO.site_id(DO.KIND_EMB, 0), 2, n_seq * Le, H) if p_hidden else None
    pid = R.roberta_pos_ids(ids, pos_pad) if pos_pad is not None else None
    if pid is not None:
        assert pid[1].tolist() == [pos_pad] * Le and pid[0, :8].tolist() == [2, 3, 4, 5, 6, 7, 8, 1] and pid.max() <= Le + 1
    got = R.embed_ln(ids, P[O.BERT + "embeddings.word_embeddings.weight"], P[O.BERT + "embeddings.position_embeddings.weight"],
                     P[O.BERT + "embeddings.token_type_embeddings.weight"][0], P[O.BERT + "embeddings.LayerNorm.weight"],
                     P[O.BERT + "embeddings.LayerNorm.bias"], 1e-12, m=m, pos_ids=pid)
    close(got, want, "embeddings")
    if m is not None:
        assert (got[m == 0] == 0).all() and (want[m == 0] == 0).all()
