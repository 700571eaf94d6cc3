"""float64 restatements of the operations that take a dropout site, for tests/test_dropout_ref_cpu.py (which ties them to
oracle/newsrec_oracle.py, itself pinned to the reference by tests/golden/stage1_cfg4_drop.npz) and for
tests/test_dropout_kernels_gpu.py (which holds the HIP kernels against them).  Plain numpy; every function takes the mask - the
fp32 multipliers 0 or 1 / (1 - p) of oracle/dropout_oracle.py - as an argument and never generates one, m = None is eval mode."""
import math

import numpy as np
from scipy.special import erf as _erf

F64 = np.float64


def _heads(x, N, L, A, d):
    return x.reshape(N, L, A, d).transpose(0, 2, 1, 3)


def _rows(x, N, L, A, d):
    return x.transpose(0, 2, 1, 3).reshape(N * L, A * d)


def attn_fwd(qkv, mask_add, rel, N, L, A, m=None, d=64):
    """qkv (N L, 3 A d) = [q | k | v], head a in columns a d .. a d + d; mask_add (N, L) additive key mask; rel (A, L, L) additive
    bias; m (N, A, L, L) multiplier on the NORMALISED probabilities (tnlrv3/modeling.py:224: the softmax runs over every key, only
    what multiplies V is masked) -> dict(q, k, v, p, m, ctx (N L, A d), lse (N, A, L) - the mask never touches it)."""
    qkv = np.asarray(qkv, F64)
    q, k, v = [_heads(qkv[:, i * A * d:(i + 1) * A * d], N, L, A, d) for i in range(3)]
    s = q @ k.transpose(0, 1, 3, 2) / math.sqrt(d) + np.asarray(mask_add, F64)[:, None, None, :] + np.asarray(rel, F64)[None]
    mx = s.max(-1, keepdims=True)
    e = np.exp(s - mx)
    den = e.sum(-1, keepdims=True)
    p = e / den
    pm = p if m is None else p * np.asarray(m, F64)
    return dict(q=q, k=k, v=v, p=p, m=None if m is None else np.asarray(m, F64), ctx=_rows(pm @ v, N, L, A, d),
                lse=(np.log(den) + mx)[..., 0], dims=(N, L, A, d))


def attn_bwd(c, dctx):
    """Backward of attn_fwd: dP = m o (dctx V^T), dV = (P o m)^T dctx, dS = P o (dP - rowsum(dP o P)), dQ = dS K / sqrt(d),
    dK = dS^T Q / sqrt(d) -> (dqkv (N L, 3 A d) = [dq | dk | dv], dS (N, A, L, L))."""
    N, L, A, d = c["dims"]
    q, k, v, p, m = c["q"], c["k"], c["v"], c["p"], c["m"]
    dch = _heads(np.asarray(dctx, F64), N, L, A, d)
    dp = dch @ v.transpose(0, 1, 3, 2)
    pm = p
    if m is not None:
        dp = dp * m
        pm = p * m
    dv = pm.transpose(0, 1, 3, 2) @ dch
    ds = p * (dp - (dp * p).sum(-1, keepdims=True))
    dq = ds @ k / math.sqrt(d)
    dk = ds.transpose(0, 1, 3, 2) @ q / math.sqrt(d)
    return np.concatenate([_rows(dq, N, L, A, d), _rows(dk, N, L, A, d), _rows(dv, N, L, A, d)], 1), ds


def gelu(x):
    x = np.asarray(x, F64)
    return x * 0.5 * (1.0 + _erf(x / math.sqrt(2.0)))


def linear_do(a, b, bias=None, m=None, res=None, act=None):
    """(A B^T + bias [-> act]) o m + res: BertSelfOutput / BertOutput = dense -> dropout -> (x + residual); the mask sits in front
    of the residual add.  a (M, K), b (N, K), bias (N), m / res (M, N)."""
    y = np.asarray(a, F64) @ np.asarray(b, F64).T
    if bias is not None:
        y = y + np.asarray(bias, F64)
    if act is not None:
        y = act(y)
    if m is not None:
        y = y * np.asarray(m, F64)
    if res is not None:
        y = y + np.asarray(res, F64)
    return y


def layer_norm(x, gamma, beta, eps):
    x = np.asarray(x, F64)
    xc = x - x.mean(-1, keepdims=True)
    return xc / np.sqrt((xc * xc).mean(-1, keepdims=True) + eps) * np.asarray(gamma, F64) + np.asarray(beta, F64)


def roberta_pos_ids(ids, pad):
    """transformers create_position_ids_from_input_ids: cumulative count of the non-pad tokens, + padding_idx; pad tokens sit on
    row padding_idx."""
    ne = (np.asarray(ids) != pad).astype(np.int64)
    return np.cumsum(ne, 1) * ne + pad


def embed_ln(ids, word, pos, type0, gamma, beta, eps, m=None, pos_ids=None):
    """word[ids] + pos[i or pos_ids] + type0 -> LayerNorm -> o m (tnlrv3/modeling.py:153-178).  ids (N, L), m (N L, H) ->
    (N L, H)."""
    N, L = ids.shape
    pe = np.asarray(pos, F64)[np.arange(L)[None, :].repeat(N, 0) if pos_ids is None else np.asarray(pos_ids)]
    y = layer_norm(np.asarray(word, F64)[ids] + pe + np.asarray(type0, F64), gamma, beta, eps).reshape(N * L, -1)
    return y if m is None else y * np.asarray(m, F64)
