"""float64 numpy restatements of what the fp32 head, loss and optimiser kernels compute (csrc/heads.hip, optim.hip, util_f32.hip):
the references of tests/test_heads_kernels_gpu.py, tied to oracle/newsrec_oracle.py by tests/test_heads_ref_cpu.py.  Everything
is computed in float64 from the inputs as given, in the layouts the entry points use (row tables + index arrays, stacked
per-model parameters), so a test can compare an output buffer with the matching array here element by element.  Line numbers
are those of the reference's model_bert.py, the ones include/tnr_hip.h cites."""
import numpy as np

F64 = np.float64


def f64(x):
    return np.asarray(x, F64)


def blend(vec, hidx, mask, pad, user_log_mask):
    """hv[b, u] = vec[hidx[b, u]] m[b, u] + pad (1 - m[b, u])  (model_bert.py:168-170), or the plain gather vec[hidx[b, u]] under
    user_log_mask (:161-166).  vec (R, D), hidx (B, U), mask (B, U), pad (D,) -> (B, U, D)."""
    hv = f64(vec)[np.asarray(hidx)]
    if user_log_mask:
        return hv
    m = f64(mask)[..., None]
    return hv * m + f64(pad)[None, None, :] * (1.0 - m)


def user_fwd(hv, mask, w1, b1, w2, b2, user_log_mask):
    """AttentionPooling.forward (model_bert.py:23-33) as UserEncoder.forward calls it (:164-166 with the mask, :173-175 without):
    e = tanh(hv W1^T + b1), a = exp(e . w2 + b2) [* m under user_log_mask], den = sum_u a + 1e-8, alpha = a / den,
    user = sum_u alpha hv.  hv (B, U, D), w1 (Q, D), b1 (Q,), w2 (Q,), b2 scalar -> dict(e, a, den, alpha, user)."""
    hv = f64(hv)
    e = np.tanh(hv @ f64(w1).T + f64(b1))
    arg = e @ f64(w2) + float(b2)
    a = np.exp(arg)
    if user_log_mask:
        a = a * f64(mask)
    den = a.sum(1) + 1e-8
    alpha = a / den[:, None]
    return dict(e=e, a=a, arg=arg, den=den, alpha=alpha, user=np.einsum("bu,bud->bd", alpha, hv))


def user_bwd(hv, mask, w1, w2, fwd, duser, user_log_mask):
    """Backward of user_fwd + blend for a given d loss / d user (B, D), per impression:
      dw_u = hv_u . duser ; da_u = alpha_u (dw_u - sum_u' alpha_u' dw_u')        (through alpha = a / (sum a + 1e-8), a = exp(.) [m])
      dpre = da_u w2_q (1 - e^2) ; dhv = alpha_u duser + dpre W1
      part_b1 = sum_u dpre ; part_w2 = sum_u da_u e ; part_b2 = sum_u da_u ; part_pad = sum_u dhv (1 - m)   [0 under user_log_mask]
      dW1 = sum_b dpre^T hv ; dslot = dhv m   [dhv under user_log_mask]: the gradient of each history SLOT, scattered by scatter().
    The fc2 bias gradient part_b2 is zero in exact arithmetic up to the 1e-8 of the normaliser: sum_u da_u = S (1 - sum alpha)."""
    hv, e, alpha, duser = f64(hv), fwd["e"], fwd["alpha"], f64(duser)
    dw = np.einsum("bud,bd->bu", hv, duser)
    da = alpha * (dw - (dw * alpha).sum(1, keepdims=True))
    dpre = da[..., None] * f64(w2)[None, None, :] * (1.0 - e * e)
    dhv = alpha[..., None] * duser[:, None, :] + dpre @ f64(w1)
    m = np.ones_like(alpha) if user_log_mask else f64(mask)
    return dict(dpre=dpre, dhv=dhv, dslot=dhv * m[..., None], dW1=np.einsum("buq,bud->qd", dpre, hv),
                part_b1=dpre.sum(1), part_w2=np.einsum("bu,buq->bq", da, e), part_b2=da.sum(1),
                part_pad=(dhv * (1.0 - m[..., None])).sum(1))


def scatter(idx, rows, R, base=None):
    """dvec[idx[k]] += rows[k] (a row named twice gets the sum of both slots) -> (dvec (R, D), sum of |terms| per element: the
    scale of the fixed-order fp32 sum's rounding bound)."""
    rows = f64(rows).reshape(-1, rows.shape[-1])
    out = np.zeros((R, rows.shape[1]), F64) if base is None else f64(base).copy()
    mag = np.abs(out)
    np.add.at(out, np.asarray(idx).reshape(-1), rows)
    np.add.at(mag, np.asarray(idx).reshape(-1), np.abs(rows))
    return out, mag


def score_fwd(vec, cidx, user):
    """score[b, c] = vec[cidx[b, c]] . user[b]  (the bmm of model_bert.py:204 / :286-287)."""
    return np.einsum("bcd,bd->bc", f64(vec)[np.asarray(cidx)], f64(user))


def score_bwd(vec, cidx, user, dscore):
    """Backward of score_fwd: dcand[b, c] = dscore[b, c] user[b] (per candidate SLOT, scattered by scatter()),
    duser[b] = sum_c dscore[b, c] vec[cidx[b, c]]."""
    dscore = f64(dscore)
    return dscore[:, :, None] * f64(user)[:, None, :], np.einsum("bc,bcd->bd", dscore, f64(vec)[np.asarray(cidx)])


def nrms_fwd(qkv, mask, use_mask, n_heads):
    """ScaledDotProductAttention.forward (model_bert.py:51-58) on projected rows qkv (B, U, 3 Dh) = [q | k | v], Dh = 16 n_heads:
    sc_ij = exp(q_i . k_j / 4) [* m_j], attn = sc / (sum_j sc + 1e-8), ctx_i = sum_j attn_ij v_j.  Raw exp, no max subtraction.
    -> dict(ctx (B, U, Dh), sc, den, attn (B, h, U, U), arg_max: the largest exponent argument)."""
    qkv = f64(qkv)
    B, U, _ = qkv.shape
    Dh = n_heads * 16
    sp = lambda t: t.reshape(B, U, n_heads, 16).transpose(0, 2, 1, 3)
    q, k, v = sp(qkv[..., :Dh]), sp(qkv[..., Dh:2 * Dh]), sp(qkv[..., 2 * Dh:])
    arg = np.einsum("bhid,bhjd->bhij", q, k) / 4.0
    sc = np.exp(arg)
    if use_mask:
        sc = sc * f64(mask)[:, None, None, :]
    den = sc.sum(-1, keepdims=True) + 1e-8
    attn = sc / den
    ctx = np.einsum("bhij,bhjd->bhid", attn, v).transpose(0, 2, 1, 3).reshape(B, U, Dh)
    return dict(ctx=ctx, q=q, k=k, v=v, sc=sc, den=den, attn=attn, arg_max=float(arg.max()))


def nrms_bwd(fwd, dctx):
    """Backward of nrms_fwd for dctx (B, U, Dh) -> dqkv (B, U, 3 Dh):
      dattn_ij = dctx_i . v_j ; dv_j = sum_i attn_ij dctx_i ; dsc = (dattn - sum_j dattn attn) / den
      ds = dsc sc / 4 (the mask factor is part of sc) ; dq_i = sum_j ds_ij k_j ; dk_j = sum_i ds_ij q_i."""
    q, k, v, attn, sc, den = (fwd[n] for n in ("q", "k", "v", "attn", "sc", "den"))
    B, nh, U, _ = q.shape
    dc = f64(dctx).reshape(B, U, nh, 16).transpose(0, 2, 1, 3)
    dattn = np.einsum("bhid,bhjd->bhij", dc, v)
    dv = np.einsum("bhij,bhid->bhjd", attn, dc)
    ds = (dattn - (dattn * attn).sum(-1, keepdims=True)) / den * sc / 4.0
    dq = np.einsum("bhij,bhjd->bhid", ds, k)
    dk = np.einsum("bhij,bhid->bhjd", ds, q)
    mg = lambda t: t.transpose(0, 2, 1, 3).reshape(B, U, nh * 16)
    return np.concatenate([mg(dq), mg(dk), mg(dv)], -1)


def log_softmax(x):
    z = f64(x) - f64(x).max(-1, keepdims=True)
    return z - np.log(np.exp(z).sum(-1, keepdims=True))


def kd_score_loss(s, ts, label, tau, coef):
    """Model.forward's score-level losses (model_bert.py:271, 288-298; kd_ce_loss :208-219) and d / d student score of
    distill + coef * target:
      CE_t = -log_softmax(ts_t)[label] ; tw = softmax_t(-CE_t) ; mix = sum_t tw_t ts_t ; pT = softmax(mix / tau)
      distill = mean_b -sum_c pT log_softmax(s / tau) ; target = mean_b -log_softmax(s)[label]
      dscore = ((softmax(s / tau) - pT) / tau + coef (softmax(s) - onehot)) / B
    s (B, C), ts (T, B, C) (T = 0: no teachers, distill = 0 and only the target term), label (B,) ->
    dict(tw (B, T), distill, target, dscore)."""
    s = f64(s)
    B, C = s.shape
    label = np.asarray(label)
    rows = np.arange(B)
    onehot = np.zeros((B, C), F64)
    onehot[rows, label] = 1.0
    ls1 = log_softmax(s)
    target = float(-ls1[rows, label].mean())
    dscore = coef * (np.exp(ls1) - onehot)
    T = 0 if ts is None else len(ts)
    tw, distill = np.zeros((B, 0), F64), 0.0
    if T:
        ts = f64(ts)
        ce = np.stack([-log_softmax(ts[t])[rows, label] for t in range(T)], -1)
        tw = np.exp(log_softmax(-ce))
        mix = np.einsum("tbc,bt->bc", ts, tw)
        pT = np.exp(log_softmax(mix / tau))
        lst = log_softmax(s / tau)
        distill = float((-(pT * lst).sum(-1)).mean())
        dscore = dscore + (np.exp(lst) - pT) / tau
    return dict(tw=tw, distill=distill, target=target, dscore=dscore / B)


def kd_embed_loss(S, P, tw, B, U, C):
    """Embedding-level KD (model_bert.py:277-284, 300-303) on the stacked rows [B U history | B C candidate | B user] (U = 0: the
    stage-1 layout [B C titles | B bodies]): row r belongs to impression b(r); a news row counts 1 / (U + C), a user row 1:
      loss = sum_t sum_r tw[b(r), t] rowscale(r) mean_d (S_r - P_tr)^2 / B
      dS = sum_t c_tr (S - P_t), dP_t = -c_tr (S - P_t), c_tr = 2 tw[b(r), t] rowscale(r) / (D B).
    S (Rtot, D), P (T, Rtot, D), tw (B, T) -> (loss, dS, dP)."""
    S, P, tw = f64(S), f64(P), f64(tw)
    D = S.shape[1]
    bidx = np.concatenate([np.repeat(np.arange(B), U), np.repeat(np.arange(B), C), np.arange(B)])
    scale = np.concatenate([np.full(B * (U + C), 1.0 / (U + C)), np.ones(B)])
    diff = S[None] - P                                           # (T, Rtot, D)
    w = tw[bidx].T * scale[None, :]                              # (T, Rtot)
    loss = float((w * (diff ** 2).mean(-1)).sum() / B)
    c = (2.0 / (D * B)) * w[..., None]
    return loss, (c * diff).sum(0), -c * diff


def segment_sum(src, order, seg):
    """out[u] = sum_{j in [seg[u], seg[u+1])} src[order[j]] ; an empty segment gives a zero row.  -> (out, sum of |terms|)."""
    src, order, seg = f64(src), np.asarray(order), np.asarray(seg)
    out = np.zeros((len(seg) - 1, src.shape[1]), F64)
    mag = np.zeros_like(out)
    for u in range(len(seg) - 1):
        rows = src[order[seg[u]:seg[u + 1]]]
        out[u], mag[u] = rows.sum(0), np.abs(rows).sum(0)
    return out, mag


def reduce_desc(src, rows, stride, ncols, dst0=None, scale=1.0):
    """One descriptor of tnr_reduce_multi: dst[c] (+)= scale * sum_r src[r * stride + c], c < ncols.  src is the flat buffer from the
    descriptor's source pointer on, dst0 the destination's earlier contents when it accumulates.  -> (dst, sum of |terms|)."""
    m = f64(src)[:(rows - 1) * stride + ncols]
    m = np.stack([m[r * stride:r * stride + ncols] for r in range(rows)], 0)
    out, mag = scale * m.sum(0), abs(scale) * np.abs(m).sum(0)
    if dst0 is not None:
        out, mag = out + f64(dst0), mag + np.abs(f64(dst0))
    return out, mag


def adam_step(p, g, m, v, vmax, bc_step, lr, b1=0.9, b2=0.999, eps=1e-8, grad_scale=1.0):
    """torch.optim.Adam (run.py:134), amsgrad when vmax is given, plain Adam when it is None; bc_step is the step number the bias
    corrections use (the number of steps actually taken, which the guarded kernel may pick below the caller's count):
      g' = grad_scale g ; m = b1 m + (1 - b1) g' ; v = b2 v + (1 - b2) g'^2 ; vm = max(vmax, v) [amsgrad] or v
      p -= lr / (1 - b1^t) * m / (sqrt(vm) / sqrt(1 - b2^t) + eps).   -> new (p, m, v, vmax)."""
    g = f64(g) * grad_scale
    m = f64(m) * b1 + (1.0 - b1) * g
    v = f64(v) * b2 + (1.0 - b2) * g * g
    vm = v if vmax is None else np.maximum(f64(vmax), v)
    p = f64(p) - lr / (1.0 - b1 ** bc_step) * (m / (np.sqrt(vm) / np.sqrt(1.0 - b2 ** bc_step) + eps))
    return p, m, v, (None if vmax is None else vm)
