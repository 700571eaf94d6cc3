"""Shared by tests/test_widths_ref_cpu.py and tests/test_encoder_widths_gpu.py: whole-training-step cases at every encoder
width EngineConfig accepts (hidden in {256, 512, 768, 1024}, head size 64, inter % 128 == 0), their oracle results, the NT GEMM
launches each case issues with the route it expects, and the gradient comparison both files use.  Imports no GPU module.

A case is chosen for the composition paths it reaches (one or two each), at the smallest shape that reaches them:
  h256_i384_l19     l32 attention, frozen layer below the trainable one (scr / scr_y), inter 128 x 3, user_log_mask, T = 2
  h512_i1152_l40    long attention (q/k/v bias through tnr_colsum), mean pooling, all layers trainable, inter 128 x 9, T = 1
  h1024_i2176_l70   chunked pooling (L > AP_LONG), K split 4 of the small fp32 GEMMs, inter 128 x 17, T = 3
  h256_i640_l33     NRMS (4 heads x 16 = news_dim), cls pooling, long attention, inter 128 x 5
  h512_i1024_l9     126 token rows: M <= 128, the unfused column sum of _ffn_bwd, one layer, inter % 256 == 0
  h1024_i2048_l24   inter % 256 == 0 at 1024 (weight gradients on 256 x 256 tiles), all layers trainable, user_log_mask
  h256_i2048_rows   5 280 token rows: the persistent NT route for the FFN-up GEMM (N = 2048) at hidden 256
  h768_control      the width every other engine test pins (test_odd_shapes_against_oracle's first shape)"""
import numpy as np

import hashinit
from schema import FULL, state_shapes
from oracle import newsrec_oracle as O

BERT = O.BERT
VOCAB, MAX_POS = 2000, 128
QPAD = 256

# tolerances of tools/fuzz_engine.py: (loss, score) relative to max(1, |ref|), gradients relative L2
TOLS = dict(fp16=(2e-3, 3e-3, 2e-2), bf16=(1.6e-2, 2.4e-2, 8e-2))
NOOP = ("self.key.bias", "att_fc2.bias", "W_K.bias")      # mathematical no-ops: the softmax / normaliser removes them
NOOP_ABS = 1e-3                                            # rounding noise only (test_training_step_matches_reference_and_oracle)
MIN_NORM = 1e-7                                            # no other gradient of the oracle is smaller (test_widths_ref_cpu.py)

# route names: "128" = 128x128, "256x128", "pp" = the persistent kernel (256x256 or 224x256 tiles), "256" = 256x256 exactly
# (column sums ride along: never the 224-row tiling).  On a 256-CU device.
WIDTH_CASES = {
    "h256_i384_l19": dict(H=256, A=4, I=384, L=19, pooling="att", nrms=0, B=3, U=7, C=3, D=64, Q=72, T=2, nl=2, tr=(1,), ulm=True,
                          routes=dict(qkv="128", attn_out="128", ffn_up_kept="128", ffn_up_frozen="128", ffn_down="128",
                                      pool_fc1="128", dgrad_pool="128", dgrad_w2="128", dgrad_w1="128", dgrad_o="128"),
                          routes_embed=dict(dgrad_qkv="128")),      # train_embeddings: the backward goes on through layer 0
    "h512_i1152_l40": dict(H=512, A=8, I=1152, L=40, pooling="mean", nrms=0, B=3, U=7, C=3, D=64, Q=72, T=1, nl=2, tr=(0, 1),
                           ulm=False,
                           routes=dict(qkv="128", attn_out="128", ffn_up_kept="128", ffn_down="128", dgrad_w2="128", dgrad_w1="128",
                                       dgrad_o="128", dgrad_qkv="128")),
    "h1024_i2176_l70": dict(H=1024, A=16, I=2176, L=70, pooling="att", nrms=0, B=3, U=7, C=3, D=64, Q=72, T=3, nl=2, tr=(1,),
                            ulm=False,
                            routes=dict(qkv="128", attn_out="128", ffn_up_kept="128", ffn_up_frozen="128", ffn_down="128",
                                        pool_fc1="128", dgrad_pool="128", dgrad_w2="128", dgrad_w1="128", dgrad_o="128")),
    "h256_i640_l33": dict(H=256, A=4, I=640, L=33, pooling="cls", nrms=4, B=3, U=7, C=3, D=64, Q=72, T=2, nl=2, tr=(0, 1), ulm=False,
                          routes=dict(qkv="128", attn_out="128", ffn_up_kept="128", ffn_down="128", dgrad_w2="128", dgrad_w1="128",
                                      dgrad_o="128", dgrad_qkv="128")),
    "h512_i1024_l9": dict(H=512, A=8, I=1024, L=9, pooling="att", nrms=0, B=2, U=5, C=2, D=128, Q=40, T=1, nl=1, tr=(0,), ulm=False,
                          routes=dict(qkv="128", attn_out="128", ffn_up_kept="128", ffn_down="128", pool_fc1="128", dgrad_pool="128",
                                      dgrad_w2="128", dgrad_w1="128", dgrad_o="128")),
    "h1024_i2048_l24": dict(H=1024, A=16, I=2048, L=24, pooling="att", nrms=0, B=2, U=5, C=2, D=128, Q=72, T=1, nl=2, tr=(0, 1),
                            ulm=True,
                            routes=dict(qkv="128", attn_out="128", ffn_up_kept="128", ffn_down="128", pool_fc1="128",
                                        dgrad_pool="128", dgrad_w2="256", dgrad_w1="128", dgrad_o="128", dgrad_qkv="128")),
    "h256_i2048_rows": dict(H=256, A=4, I=2048, L=30, pooling="att", nrms=0, B=4, U=40, C=4, D=64, Q=72, T=2, nl=2, tr=(1,),
                            ulm=False,
                            routes=dict(qkv="128", attn_out="128", ffn_up_kept="pp", ffn_up_frozen="pp", ffn_down="128",
                                        pool_fc1="128", dgrad_pool="128", dgrad_w2="256", dgrad_w1="128", dgrad_o="128")),
    "h768_control": dict(H=768, A=12, I=3072, L=17, pooling="att", nrms=0, B=3, U=13, C=3, D=64, Q=40, T=2, nl=2, tr=(1,), ulm=True,
                         routes=dict(qkv="128", attn_out="128", ffn_up_kept="128", ffn_up_frozen="128", ffn_down="128",
                                     pool_fc1="128", dgrad_pool="128", dgrad_w2="256", dgrad_w1="128", dgrad_o="128")),
}
PORT_CASES = [n for n, c in WIDTH_CASES.items() if c["pooling"] == "att" and not c["nrms"]]     # what oracle/torch_port.py covers


def rows(c):
    """Token rows of the case's encoder pass."""
    return c["B"] * (c["U"] + c["C"]) * c["L"]


def dims(c):
    return dict(FULL, H=c["H"], A=c["A"], I=c["I"], Q=c["Q"], vocab=VOCAB, max_pos=MAX_POS)


def _tokens(rs, n, L):
    out = np.zeros((n, 2 * L), np.int64)
    for r in range(n):
        k = rs.randint(1, L + 1)
        out[r, :k] = rs.randint(1, VOCAB, k)
        out[r, L:L + k] = 1
    return out


def build_case(name, seed=91):
    """-> (P weights, cfg of the oracle, EngineConfig keyword arguments, inputs (hist, mask, cand, label, th, tc)): hash-initialised
    weights, random-length titles from a fixed RandomState, one history row fully masked when B > 1."""
    c = WIDTH_CASES[name]
    B, U, C, L, D, T_ = c["B"], c["U"], c["C"], c["L"], c["D"], c["T"]
    P = hashinit.init_state_dict(seed, state_shapes(dims(c), c["nl"], D, T_, c["pooling"], c["nrms"]))
    cfg = dict(n_layers=c["nl"], heads=c["A"], trainable_layers=list(c["tr"]), user_log_mask=c["ulm"], temperature=1.5, coef=0.3,
               pooling=c["pooling"], nrms_heads=c["nrms"])
    rs = np.random.RandomState(5)
    hist, cand = _tokens(rs, B * U, L).reshape(B, U, 2 * L), _tokens(rs, B * C, L).reshape(B, C, 2 * L)
    mask = (rs.rand(B, U) > 0.3).astype(np.float32)
    mask[0, :] = 0 if B > 1 else 1
    label = rs.randint(0, C, B)
    th = [rs.randn(B, U, D).astype(np.float32) * 0.3 for _ in range(T_)]
    tc = [rs.randn(B, C, D).astype(np.float32) * 0.3 for _ in range(T_)]
    kw = dict(n_layers=c["nl"], trainable_layers=c["tr"], hidden=c["H"], heads=c["A"], inter=c["I"], num_teachers=T_,
              user_log_length=U, npratio=C - 1, num_words=L, news_dim=D, news_query=c["Q"], user_query=c["Q"], user_log_mask=c["ulm"],
              temperature=1.5, coef=0.3, pooling=c["pooling"], nrms_heads=c["nrms"], vocab=VOCAB, max_pos=MAX_POS)
    return P, cfg, kw, (hist, mask, cand, label, th, tc)


_CASE, _ORACLE = {}, {}


def case(name):
    """build_case(name), built once and shared (never modified)."""
    if name not in _CASE:
        _CASE[name] = build_case(name)
    return _CASE[name]


def oracle(name):
    """-> (losses [distill, target, emb], student scores, {key: gradient}) of the numpy oracle, computed once per case."""
    if name not in _ORACLE:
        P, cfg, _, inp = case(name)
        out = O.model_fwd(P, cfg, *inp)
        G = O.model_bwd(P, cfg, out)
        _ORACLE[name] = (np.array([out["distill_loss"], out["target_loss"], out["emb_loss"]], np.float64), out["student_score"], G)
    return _ORACLE[name]


def nt_launches(name, train_embeddings=False):
    """(launch name, N, K, epilogue flag names) of every NT GEMM a forward + backward of the case issues (engine.py: _layer_fwd,
    _head_fwd, _head_bwd_dgrad, _ffn_bwd, _att_bwd, _qkv_dgrad).  M = rows(case) for all of them.  train_embeddings keeps every
    layer resident and runs the backward down to the embeddings (expected routes: the case's routes + routes_embed)."""
    c = WIDTH_CASES[name]
    H, I, M = c["H"], c["I"], rows(c)
    lo = 0 if train_embeddings else min(c["tr"])
    out = [("qkv", 3 * H, H, ("BIAS",)), ("attn_out", H, H, ("BIAS", "RES")), ("ffn_up_kept", I, H, ("BIAS", "GELU", "AUXOUT")),
           ("ffn_down", H, I, ("BIAS", "RES"))]
    if lo > 0:
        out.append(("ffn_up_frozen", I, H, ("BIAS", "GELU")))
    if c["pooling"] == "att":
        out += [("pool_fc1", QPAD, H, ("BIAS", "TANH", "OUTF32")), ("dgrad_pool", H, QPAD, ("RES",))]
    out += [("dgrad_w2", I, H, ("MULDGELU", "COLSUM") if M > 128 else ("MULDGELU",)), ("dgrad_w1", H, I, ("RES",)), ("dgrad_o", H, H, ())]
    if c["nl"] - 1 > lo or train_embeddings:
        out.append(("dgrad_qkv", H, 3 * H, ("RES",)))
    return out


def exempt(name, key):
    """None for a gradient held to the relative bound; else how the key is checked instead: "noop" (NOOP: |g| < NOOP_ABS) or "zero"
    (pad_doc under user_log_mask: the history is masked instead of blended, the parameter is unused, both sides exactly 0)."""
    if key.endswith(NOOP):
        return "noop"
    if key.endswith("pad_doc") and WIDTH_CASES[name]["ulm"]:
        return "zero"
    return None


def rel_l2(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.sqrt(((got - ref) ** 2).sum()) / np.sqrt((ref ** 2).sum()))


def compare_grads(name, keys, got_of, G, gtol):
    """Every key of `keys` against the oracle's gradients G: relative L2 under gtol, no key passed over - the exempt ones
    (exempt()) are checked absolutely.  got_of(key) -> numpy array.  -> (worst relative error, its key, [keys out of bound])."""
    worst, wk, bad = 0.0, "", []
    for k in keys:
        got, ref = np.asarray(got_of(k)), G[k]
        assert got.shape == ref.shape, (k, got.shape, ref.shape)
        how = exempt(name, k)
        if how == "noop":
            if not np.abs(got).max() < NOOP_ABS:
                bad.append(k)
            continue
        if how == "zero":
            if np.abs(got).max() != 0.0 or np.abs(ref).max() != 0.0:
                bad.append(k)
            continue
        err = rel_l2(got, ref)
        if err > worst:
            worst, wk = err, k
        if not err < gtol:
            bad.append(k)
    return worst, wk, bad
