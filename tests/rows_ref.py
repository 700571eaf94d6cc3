"""float64 numpy restatements of what the row kernels on the 16-bit activations compute (csrc/norm_embed.hip, csrc/attpool.hip with its
fp32 stages in heads.hip, tnr_relpos_table in util_f32.hip), the error bound of every output, and the input sets of
tests/test_rows_kernels_gpu.py.  tests/test_rows_ref_cpu.py ties the restatements to oracle/newsrec_oracle.py and shows, without a
GPU, that a correct fp32 evaluation rounded once to the 16-bit type passes every bound on every one of those input sets.

Inputs are the 16-bit-rounded values the kernel sees (r16); everything is computed in float64 from them.

Bounds.  |got - ref| <= u16 |ref| + tiny16  (16-bit outputs only)  +  c * 2^-23 * mag
  u16     2^-8 (bf16) / 2^-11 (fp16): one round-to-nearest of a p-bit significand.
  tiny16  half the spacing of the type's subnormals (2^-25 for fp16, 2^-134 for bf16): below the smallest normal the rounding error
          is absolute.  An fp16 LayerNorm output lands below 6.1e-5 about once in 10^4 elements.
  mag     the same formula with every term replaced by its absolute value, so cancellation shows.
  c       the number of fp32 operations on the path, 2^-23 each (twice the unit roundoff).  A sum of n terms counts as n, with
          three exceptions.  The column sums over M rows (tnr_colsum; dgamma, dbeta and dxsum of the LayerNorm backward) count
          min(M, depth), depth the additions on the path of any one term through the kernel's chains and the row reduction
          behind it (colsum_depth, ln_bwd_depth: 150 for tnr_colsum at M = 32773, 33 for the backward at M = 32777): counted as
          M, the bound at M = 32777 is 100 on a sum of magnitude 500 and a lost 128-row block (about 11) passes.  The
          H-term dot product dw of the pooling backward counts AP_DW_DEPTH(H) = 4 ceil(H / 256) + 6 for the same reason: as H + 1,
          dw2_part's bound at L = 512 is twice one token's whole contribution.  And the three
          row sums of a LayerNorm (mean, mean(g), mean(g xh)) count LN_DEPTH(H) = H / 32 + 5, the additions
          on the path of any one term when half a wave owns a row (a chain of H / 32 in the lane, a 5-level butterfly).  Counting
          them as H would put the bound of y on a row of mean 30 and spread 0.5 at 1025 * 2^-23 * 30 * rstd |gamma| = 8e-3, above
          the flat 1.5e-3 the fp16 output is held to in tests/test_kernels_gpu.py; the embedding kernel's wave per row is shallower.
  rsqrtf  2 ulp (the OpenCL bound, which the device library's rsqrt meets): rstd is relative (H / 2 + 4) 2^-23 - H + 4 operations
          for the variance (H squares summed, the difference and the product in each, the divide, the eps), halved by the square
          root, + 2 - plus the mean's share (an error d of the mean adds d^2 to the variance).
  Behind __expf nothing is derived: alpha, den and nv keep rtol 1e-4 with floor 1e-5 of the tensor's largest magnitude (FWD / FLOOR
  of tests/test_heads_kernels_gpu.py).  db2_part is a cancelling sum (zero in exact arithmetic) and is held absolutely against
  2e-4 of dw2_part's largest magnitude, as tests/test_kernels_gpu.py::test_attpool_long_equals_the_one_workgroup_kernels does.
Line numbers are those of the reference's model_bert.py / tnlrv3/modeling.py, the ones include/tnr_hip.h cites."""
import numpy as np

F64 = np.float64
U23 = 2.0 ** -23
U16 = {"bf16": 2.0 ** -8, "f16": 2.0 ** -11}
TINY16 = {"bf16": 2.0 ** -134, "f16": 2.0 ** -25}
KINDS = ("bf16", "f16")
SFX = {"bf16": "", "f16": "_f16"}
FWD, FLOOR, DB2 = 1e-4, 1e-5, 2e-4
EPS = 1e-12


def f64(x):
    return np.asarray(x, F64)


def tdtype(kind):
    import torch
    return torch.bfloat16 if kind == "bf16" else torch.float16


def r16(x, kind):
    """Round (through fp32) to the 16-bit type with torch's CPU cast -> float64 of the rounded values."""
    import torch
    x32 = np.ascontiguousarray(np.asarray(x, np.float32))
    return torch.from_numpy(x32).to(tdtype(kind)).float().numpy().astype(F64)


def out16(ref, kind, fp):
    """Bound of a 16-bit output whose unrounded fp32 value is within `fp` of ref."""
    return U16[kind] * np.abs(ref) + TINY16[kind] + fp


def LN_DEPTH(H):
    return H // 32 + 5


# ------------------------------------------------------------------------------------------------ LayerNorm
def ln_fwd(x, gamma, beta, eps=EPS, xerr=None):
    """tnlrv3/modeling.py:153-178's BertLayerNorm: y = (x - mean) rstd gamma + beta, rstd = 1 / sqrt(var + eps), var the biased
    variance about the mean; eps as the fp32 the entry point takes.  x (M, H) -> dict(y, mean, rstd) and the fp32 parts of their
    bounds b_mean, b_rstd, fp_y.  xerr: absolute error x already carries (the embedding kernel's two additions)."""
    x, g, b = f64(x), f64(gamma), f64(beta)
    H = x.shape[-1]
    mean = x.mean(-1)
    xc = x - mean[:, None]
    rstd = 1.0 / np.sqrt((xc * xc).mean(-1) + float(np.float32(eps)))
    y = xc * rstd[:, None] * g + b
    ex = np.zeros_like(x) if xerr is None else f64(xerr)
    # mean: LN_DEPTH additions and the divide on sum|x| / H, + what x carries
    b_mean = (LN_DEPTH(H) + 1) * U23 * np.abs(x).mean(-1) + ex.mean(-1)
    if xerr is None:      # a row of H <= 1024 equal 16-bit values: every partial sum k v has at most 11 + 11 significant bits and is
        b_mean = np.where((xc == 0).all(-1), 0.0, b_mean)      # exact in fp32 in any order, and so is the divide: mean = v
    # rstd: see the module docstring; an error d in every centred element moves the variance by 2 mean(|xc| d)
    rel = (H / 2 + 4) * U23 + 0.5 * (b_mean * rstd) ** 2 + rstd ** 2 * (np.abs(xc) * (ex + ex.mean(-1)[:, None])).mean(-1)
    b_rstd = rstd * rel
    # y: the errors of mean, rstd and x carried through (the cancellation in x - mean shows there), + 4 operations (the
    # subtraction, whose error is relative to its result, two products, the addition) on |x - mean| rstd |gamma| + |beta|
    fp_y = (np.abs(g) * ((b_mean[:, None] + ex) * rstd[:, None] + np.abs(xc) * b_rstd[:, None])
            + 4 * U23 * (np.abs(xc) * rstd[:, None] * np.abs(g) + np.abs(b)))
    return dict(y=y, mean=mean, rstd=rstd, b_mean=b_mean, b_rstd=b_rstd, fp_y=fp_y)


def _cdiv(a, b):
    return -(-a // b)


def reduce_rows_depth(rows, n):
    """Additions on the path of one term through tnr_reduce_rows over `rows` rows of n columns (csrc/util_f32.hip): narrow
    outputs a chain per thread and an 8-level tree; tall inputs chunks summed in place (four row lanes, combined in 2) and the
    chunk rows the same way; else one level."""
    colblk = _cdiv(n, 64)
    if n < 64 and rows >= 256:
        return _cdiv(rows, 256) + 8
    if rows >= 128 and colblk < 512:
        chunks = max(min(1024 // colblk, rows // 16), 2)
        chunk = _cdiv(rows, chunks)
        return _cdiv(chunk, 4) + 2 + _cdiv(_cdiv(rows, chunk), 4) + 2
    return _cdiv(rows, 4) + 2


def ln_bwd_depth(M, H):
    """A half wave's chain over its rows of the block (32-row blocks below M = 32768, 128 from there on), the other half wave,
    the four waves, then the reduction of the partial rows (H or, dgamma and dbeta adjacent, 2 H columns: the deeper)."""
    rows = 128 if M >= 32768 else 32
    nblk = _cdiv(M, rows)
    return rows // 8 + 1 + 3 + max(reduce_rows_depth(nblk, H), reduce_rows_depth(nblk, 2 * H))


def colsum_depth(M, N, batch=1):
    """A row lane's chain (64-row blocks below M = 32768, 512 from there on, four lanes), their combine in 3, the reduction."""
    rpb = 512 if M >= 32768 else 64
    return rpb // 4 + 3 + reduce_rows_depth(_cdiv(M, rpb), batch * N)


def ln_bwd(dy, x, mean, rstd, gamma, kind, mask=None):
    """Backward of ln_fwd from the saved statistics AS GIVEN (fp32 values): xh = (x - mean) rstd, g = dy gamma,
    dx = rstd (g - mean(g) - xh mean(g xh)), dgamma = sum_m dy xh, dbeta = sum_m dy; dxm = dx mask (the masked second output of
    tnr_ln_bwd_do, mask the 0 or 1 / (1 - p) multipliers); dxsum = column sums of the ROUNDED dxm (of the rounded dx without a
    site): what the weight-gradient kernels will see.  -> the outputs and the fp32 parts of their bounds."""
    dy, x, mean, rstd, gm = f64(dy), f64(x), f64(mean)[:, None], f64(rstd)[:, None], f64(gamma)
    M, H = x.shape
    xh = (x - mean) * rstd
    g = dy * gm
    s1, s2 = g.mean(-1, keepdims=True), (g * xh).mean(-1, keepdims=True)
    dx = rstd * (g - s1 - xh * s2)
    # s1: LN_DEPTH additions, the divide, the product in g ; s2: + the two operations of xh and the product g xh
    b_s1 = (LN_DEPTH(H) + 2) * U23 * np.abs(g).mean(-1, keepdims=True)
    b_s2 = (LN_DEPTH(H) + 5) * U23 * np.abs(g * xh).mean(-1, keepdims=True)
    # dx: 7 operations (xh 2, g 1, xh s2 1, two subtractions, the product with rstd) on rstd (|g| + |mean g| + |xh| |mean(g xh)|)
    fp_dx = rstd * (b_s1 + np.abs(xh) * b_s2) + 7 * U23 * rstd * (np.abs(g) + np.abs(s1) + np.abs(xh) * np.abs(s2))
    cnt = min(M, ln_bwd_depth(M, H))
    out = dict(dx=dx, fp_dx=fp_dx, xh=xh, count=cnt,
               dgamma=(dy * xh).sum(0), b_dgamma=(cnt + 3) * U23 * np.abs(dy * xh).sum(0),    # each term a product of a 2-operation xh
               dbeta=dy.sum(0), b_dbeta=cnt * U23 * np.abs(dy).sum(0))
    second = dx
    if mask is not None:
        m = f64(mask)
        out["dxm"], out["fp_dxm"] = dx * m, (fp_dx + U23 * np.abs(dx)) * m                    # one more product
        second = out["dxm"]
    s16 = r16(second, kind)
    out["dxsum"] = s16.sum(0)
    # against the sums of the kernel's OWN rounded output the bound is colsum_bound; against this one, every element of that
    # output may also sit one rounding away from the reference's: its bound and the rounding of the reference, summed
    fp = out["fp_dxm"] if mask is not None else fp_dx
    out["b_dxsum"] = colsum_bound(s16, cnt) + (out16(second, kind, fp) + out16(second, kind, 0.0)).sum(0)
    return out


def colsum_bound(rounded, count):
    """A fixed-order fp32 column sum against the float64 sum: count * 2^-23 * sum|x|."""
    return count * U23 * np.abs(f64(rounded)).sum(0)


LN_H = (256, 512, 768, 1024)
LN_M = (1, 7, 8, 9, 31, 32, 33, 65)
LN_TALL = (32767, 32768, 32777)
LN_DO = [(H, M) for H in (256, 1024) for M in (9, 33)]
NAN_ROWS = 8
CONST = (3.25, -1.5, 0.0)


def ln_rows(M, H, seed, n_kinds):
    """Row i is of kind (i + M) % n_kinds: 0 N(0, 2); 1 mean 30, sd 0.5; 2 N(0, 2) with one element at 60; 3 a constant."""
    rs = np.random.RandomState(seed)
    x = rs.standard_normal((M, H)) * 2.0
    kind = (np.arange(M) + M) % n_kinds
    for i in np.nonzero(kind == 1)[0]:
        x[i] = 30.0 + 0.5 * rs.standard_normal(H)
    for i in np.nonzero(kind == 2)[0]:
        x[i, rs.randint(H)] = 60.0
    for i in np.nonzero(kind == 3)[0]:
        x[i] = CONST[(i // 4) % len(CONST)]
    return x, kind


def ln_case(M, H, kind, bwd):
    """The LayerNorm input set of (M, H, build): forward cases have rows of all four kinds, backward cases leave the constant
    rows out (their rstd is 1e6).  x, dy rounded to the type; gamma, beta fp32."""
    rs = np.random.RandomState(1000 + H + M)
    x, rk = ln_rows(M, H, 2000 + H + M, 3 if bwd else 4)
    return dict(x=r16(x, kind), dy=r16(rs.standard_normal((M, H)), kind), rk=rk,
                g=(1.0 + 0.1 * rs.standard_normal(H)).astype(np.float32), b=(0.1 * rs.standard_normal(H)).astype(np.float32))


# ------------------------------------------------------------------------------------------------ embedding + LayerNorm + mask
def embed_ln(ids, word, pos, type0, gamma, beta, eps=EPS):
    """word[id] + pos[i] + type0 -> LayerNorm (tnlrv3/modeling.py:153-178).  ids (N, L) -> ln_fwd's dict over (N L, H) rows; the
    two additions in front count 2 * 2^-23 on |word| + |pos| + |type0|."""
    N, L = ids.shape
    a, b, d = f64(word)[ids], f64(pos)[np.arange(L)][None], f64(type0)[None, None]
    H = a.shape[-1]
    xerr = 2 * U23 * (np.abs(a) + np.abs(b) + np.abs(d))
    return ln_fwd((a + b + d).reshape(N * L, H), gamma, beta, eps, xerr=xerr.reshape(N * L, H))


def mask_add(mask):
    """(1 - mask) * -10000 (tnlrv3/modeling.py:446-454), exact in fp32."""
    return ((np.float32(1.0) - np.asarray(mask, np.float32)) * np.float32(-10000.0)).astype(np.float32)


EMBED_NL = ((1, 1), (3, 7), (2, 32), (2, 33), (1, 512))
VOCAB = 11


def embed_case(N, L, H):
    """ids with 0 and VOCAB - 1; the last of N >= 2 sequences all pad; tables fp32, one NaN row behind `word`, NaN in position
    rows >= L.  `table` (R, 2 L) int32 and `nidx` for the indexed form: repeats, and the table's last row."""
    rs = np.random.RandomState(3000 + 7 * N + L + H)
    ids = rs.randint(0, VOCAB, (N, L))
    ids.flat[-1] = 0
    ids.flat[0] = VOCAB - 1                        # (1, 1): the row in front of the NaN row
    mask = (rs.rand(N, L) > 0.3).astype(np.int64)
    if N >= 2:
        mask[N - 1] = 0
    word = np.full((VOCAB + 1, H), np.nan, np.float32)
    word[:VOCAB] = rs.standard_normal((VOCAB, H))
    pos = np.full((512, H), np.nan, np.float32)
    pos[:L] = rs.standard_normal((L, H))
    R = N + 2
    table = np.concatenate([rs.randint(0, VOCAB, (R, L)), (rs.rand(R, L) > 0.3).astype(np.int64)], 1).astype(np.int32)
    table[:N] = np.concatenate([ids, mask], 1)
    nidx = np.array([R - 1] + [0] * (N > 1) + [rs.randint(R) for _ in range(max(N - 2, 0))], np.int32)[:N]
    if N >= 3:
        nidx[2] = nidx[1]
    return dict(ids=ids, mask=mask, word=word, pos=pos, type0=rs.standard_normal(H).astype(np.float32),
                g=(1.0 + 0.1 * rs.standard_normal(H)).astype(np.float32), b=(0.1 * rs.standard_normal(H)).astype(np.float32),
                table=table, nidx=nidx)


# ------------------------------------------------------------------------------------------------ cls / mean pooling
def pool_fwd(y, mean):
    """model_bert.py:130-135: token 0, or the mean over ALL L positions.  y (n, L, H) -> nv (n, H) and its bound: cls copies
    (bound 0); the mean is L additions and, at 2^-24 each, the rounding of 1 / L and the product with it, on sum|y| / L."""
    y = f64(y)
    L = y.shape[1]
    if not mean:
        return y[:, 0], np.zeros_like(y[:, 0])
    return y.mean(1), (L + 1) * U23 * np.abs(y).mean(1)


def pool_bwd(dnv, L, mean):
    """-> dy (n, L, H) unrounded and the fp32 part of its bound (the rounding of 1 / L and the product; cls: none)."""
    g = f64(dnv)[:, None, :]
    if mean:
        dy = np.repeat(g / L, L, 1)
        return dy, 2 * U23 * np.abs(dy)
    dy = np.concatenate([g, np.zeros((g.shape[0], L - 1, g.shape[2]))], 1)
    return dy, np.zeros_like(dy)


POOL_H, POOL_L, POOL_N = (4, 256, 1024, 1028), (1, 2, 30), (1, 5)


def pool_case(n, L, H, kind):
    rs = np.random.RandomState(4000 + n + L + H)
    return r16(rs.standard_normal((n, L, H)), kind), rs.standard_normal((n, H)).astype(np.float32)


# ------------------------------------------------------------------------------------------------ column sums
COLSUM_M, COLSUM_N = (1, 3, 4, 5, 63, 64, 65, 129), (4, 252, 256, 260, 772)
COLSUM_SHAPES = [(M, N) for M in COLSUM_M for N in COLSUM_N] + [(32768 + 5, 4), (3, 5 * 256 * 4 + 4)]
COLSUM_BATCHED = [(1, 5, 260), (3, 5, 260), (3, 65, 256), (3, 129, 4)]


def colsum(x, out0=None):
    """x (M, N) [(batch, M, N)] -> column sums (+ out0 under accumulate) and min(M, colsum_depth) [+ 1] * 2^-23 * (sum|x|
    [+ |out0|])."""
    x = f64(x)
    s, mag = x.sum(-2), np.abs(x).sum(-2)
    n = min(x.shape[-2], colsum_depth(x.shape[-2], x.shape[-1], x.shape[0] if x.ndim == 3 else 1))
    if out0 is not None:
        s, mag, n = s + f64(out0), mag + np.abs(f64(out0)), n + 1
    return s, n * U23 * mag


def colsum_case(M, N, kind, batch=1):
    """kind "f32": fp32 input as it is; else rounded to the type."""
    rs = np.random.RandomState(5000 + M % 1000 + N + batch)
    x = rs.standard_normal((batch, M, N)).astype(np.float32)
    x = f64(x) if kind == "f32" else r16(x, kind)
    return x, rs.standard_normal((batch, N)).astype(np.float32)


# ------------------------------------------------------------------------------------------------ additive-attention pooling
def attpool_fwd(y, e, w2, b2):
    """model_bert.py:27-33: a = exp(e . w2 + b2) (raw exp, no max subtraction), den = sum_i a + 1e-8, alpha = a / den,
    nv = sum_i alpha_i y_i.  y (n, L, H), e (n, L, Q) = tanh(fc1), w2 (Q,), b2 scalar."""
    y, e = f64(y), f64(e)
    a = np.exp(e @ f64(w2) + float(b2))
    den = a.sum(1) + 1e-8
    alpha = a / den[:, None]
    return dict(alpha=alpha, den=den, nv=np.einsum("nl,nlh->nh", alpha, y))


def AP_DW_DEPTH(H):
    """The additions on the path of one term of dw_i = dnv . y_i in either pooling form: a wave per token, a lane's chain of four
    columns per 256 of H, the 6-level butterfly."""
    return 4 * _cdiv(H, 256) + 6


def attpool_bwd(y, e, w2, alpha, dnv, kind):
    """Backward from the fp32 alpha AS GIVEN: dw_i = dnv . y_i, S = sum_i alpha_i dw_i, da_i = alpha_i (dw_i - S) (the gradient of
    the fc2 output of token i), dy_direct = alpha_i dnv, dpre = da_i w2 (1 - e^2), per sequence dw2_part = sum_i da_i e_i,
    db2_part = sum_i da_i, db1_part = sum_i of the ROUNDED dpre.  -> the outputs (dy_direct, dpre unrounded) and the fp32 parts
    of their bounds."""
    y, e, w2, al, g = f64(y), f64(e), f64(w2), f64(alpha), f64(dnv)
    n, L, H = y.shape
    dw = np.einsum("nlh,nh->nl", y, g)
    b_dw = (AP_DW_DEPTH(H) + 1) * U23 * np.einsum("nlh,nh->nl", np.abs(y), np.abs(g))   # each term a product
    S = (dw * al).sum(1, keepdims=True)
    b_S = (al * b_dw).sum(1, keepdims=True) + (L + 1) * U23 * np.abs(dw * al).sum(1, keepdims=True)
    da = al * (dw - S)
    b_da = al * (b_dw + b_S) + 2 * U23 * al * (np.abs(dw) + np.abs(S))                   # the subtraction and the product
    dpre = da[..., None] * w2 * (1.0 - e * e)
    # 4 operations (two products, e e, 1 - e e) on |da| |w2| (1 + e^2)
    fp_dpre = b_da[..., None] * np.abs(w2) * (1.0 - e * e) + 4 * U23 * np.abs(da)[..., None] * np.abs(w2) * (1.0 + e * e)
    dyd = al[..., None] * g[:, None, :]
    return dict(dy_direct=dyd, fp_dy_direct=U23 * np.abs(dyd), dpre=dpre, fp_dpre=fp_dpre, da=da,
                dw2_part=np.einsum("nl,nlq->nq", da, e),
                b_dw2_part=np.einsum("nl,nlq->nq", b_da, np.abs(e)) + (L + 1) * U23 * np.einsum("nl,nlq->nq", np.abs(da), np.abs(e)),
                db2_part=da.sum(1), db1_part=r16(dpre, kind).sum(1),
                # as b_dxsum of ln_bwd: L terms, and every rounded element one rounding away from the reference's
                b_db1_part=L * U23 * np.abs(dpre).sum(1) + (out16(dpre, kind, fp_dpre) + out16(dpre, kind, 0.0)).sum(1))


AP_N = 3
AP_REAL = (768, 200, 256, 256)                                   # H, Q, lde, lddpre
AP_ODD = ((4, 1, 1, 1), (260, 64, 72, 64), (1028, 65, 208, 320))
AP_L_ONE, AP_L_LONG, AP_L_ODD = (1, 3, 4, 5, 31, 32, 33, 256, 257, 512), (1, 63, 64, 65, 127, 128, 129, 257, 512), (5, 129)


def attpool_cases(long):
    return [(L,) + AP_REAL for L in (AP_L_LONG if long else AP_L_ONE)] + [(L,) + s for s in AP_ODD for L in AP_L_ODD]


def attpool_case(L, H, Q, kind):
    """y 16-bit, e = tanh(N(0, 0.7)) as fp32, w2 ~ 0.2 N(0, 1): the exponent stays within a few units."""
    rs = np.random.RandomState(6000 + L + H + Q)
    n = AP_N
    return dict(y=r16(rs.standard_normal((n, L, H)), kind), e=np.tanh(0.7 * rs.standard_normal((n, L, Q))).astype(np.float32),
                w2=(0.2 * rs.standard_normal(Q)).astype(np.float32), b2=np.float32(0.05 * rs.standard_normal()),
                dnv=rs.standard_normal((n, H)).astype(np.float32))


# ------------------------------------------------------------------------------------------------ rel-pos table, shadow cast
RELPOS_L, RELPOS_A = (1, 31, 32, 33, 64, 91, 92, 129, 512), (1, 3, 12)
RELPOS_EDGES = ((7, 8), (11, 12), (15, 16), (22, 23), (31, 32), (45, 46), (63, 64), (90, 91))


def relpos_table(weight, L):
    from oracle import newsrec_oracle as O
    return O.relpos_bias_table(np.asarray(weight, np.float32), L)


SHADOW_SHAPES = ((1, 1), (31, 33), (32, 32), (33, 50), (200, 768), (768, 96))


def shadow_source(rows, cols, kind, seed):
    """fp32 source: N(0, 1), and from the front (as far as the size allows) exact ties between two 16-bit neighbours of both
    parities, -0.0, values below the type's normal range, and for fp16 a value above 65504."""
    x = np.random.RandomState(seed).standard_normal(rows * cols).astype(np.float32)
    if kind == "bf16":      # 1 + 2^-8 (tie, even below), 1 + 3 2^-8 (tie, even above), subnormals of bf16 = of fp32
        bits = [0x80000000, 0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000, 0x00400000, 0x00008000, 0x80018000, 0x3F808001, 0x3F807FFF]
    else:                   # 1 + 2^-11, 1 + 3 2^-11, 2^-15, 2^-24 + 2^-25 (tie of two subnormals), 2^-25 (tie with 0), 65520, 70000, 65519
        bits = [0x80000000, 0x3F801000, 0x3F803000, 0xBF801000, 0xBF803000, 0x38000000, 0x33C00000, 0x33000000, 0x477FF000, 0x4788B800, 0x477FEF00]
    sp = np.array(bits, np.uint32).view(np.float32)
    k = min(len(sp), x.size)
    x[:k] = sp[:k]
    return x.reshape(rows, cols)


def shadow_cast(src, kind):
    """The 16-bit copy as raw int16 bits: torch's CPU cast of the fp32 source (round to nearest even)."""
    import torch
    return torch.from_numpy(np.ascontiguousarray(src, np.float32)).to(tdtype(kind)).view(torch.int16).numpy()


def ln_stats32(f):
    """(M, 2) fp32 [mean | rstd]: the statistics a backward call is handed."""
    return np.stack([f["mean"], f["rstd"]], 1).astype(np.float32)


def ceil32(L):
    return (L + 31) // 32 * 32
