"""The kernels that take a dropout site, one by one, against the float64 references of tests/dropout_ref.py (tied to the oracle by
tests/test_dropout_ref_cpu.py).  Masks always come from oracle/dropout_oracle.py, never from a tnr_dropout_mask* dump.

  * attention (tnr_attn_l32_fwd_do / _bwd_do, tnr_attn_long_fwd_do / _bwd_do): the APPLIED mask read back element by element.  The
    head size is 64, so a one-hot operand over a 64-wide window w turns an output into a copy of one 64-column slab of an inner
    matrix: V one-hot -> ctx = (P o m)[:, window], dctx one-hot -> dV = (P o m)[window, :]^T (the per-key accessor of the dK / dV
    kernel), K one-hot -> dq = dS[:, window] / 8 (the dQ kernel), Q one-hot -> dk = dS[window, :]^T / 8 (the key-tile kernel).  The
    zero pattern of the first two is compared with the oracle mask exactly, for every (sequence, head, query, key);
  * attention under realistic inputs (padding, an all-pad and a half-padded sequence): ctx, lse, dqkv, the fused bias partials,
    run-to-run determinism, another forward call -> other masks;
  * tnr_gemm_nt_do on each of its four routes; tnr_embed_ln_fwd_do / _indexed_do with a site and / or a pos_ids table.

Bounds: those of the eval-mode tests of the same kernels in tests/test_kernels_gpu.py (attention 2e-3 / 3e-3 [long: 4e-3] fp16 and
2e-2 / 3e-2 bf16 forward / backward, backward relative to the reference's largest magnitude; GEMM rtol 1e-2 / atol 2e-2;
embeddings 1.5e-3 / 1e-2), times 1 / (1 - p): kept values grow by that factor and a 16-bit rounding is relative.  The parity tests
also run with a p = 0 site (the eval kernels, bit for bit): the rounding floor of these inputs.  Every comparison prints its
largest error and that error as a fraction of its bound (EXPERIMENTS.md item 59 records them)."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import dropout_ref as R                        # noqa: E402
import tnr_hip as T                            # noqa: E402
from oracle import dropout_oracle as DO       # noqa: E402
from oracle import newsrec_oracle as O        # noqa: E402

DEV = "cuda:0"
SEED, LAYER, CALL = 0x5EED0002, 2, 5          # a site with a non-zero layer and forward-call number
BUILDS = {"bf16": (torch.bfloat16, ""), "fp16": (torch.float16, "_f16")}
D = 64
SHAPES = {"l32": [(3, 30, 12), (2, 32, 2), (5, 7, 3), (1, 1, 1)],
          "long": [(2, 24, 3), (2, 33, 2), (1, 128, 12), (2, 200, 2), (1, 512, 2)]}
ATTN_CASES = [(k,) + s for k in ("l32", "long") for s in SHAPES[k]]
# (forward, backward) of test_attention_fwd_bwd / test_attention_long_fwd_bwd
ATTN_TOL = {"l32": {"fp16": (2e-3, 3e-3), "bf16": (2e-2, 3e-2)}, "long": {"fp16": (2e-3, 4e-3), "bf16": (2e-2, 3e-2)}}
EMB_TOL = {"fp16": 1.5e-3, "bf16": 1e-2}
GEMM_RTOL, GEMM_ATOL = 1e-2, 2e-2


def rnd(shape, seed, scale=1.0):
    return (np.random.RandomState(seed).standard_normal(shape) * scale).astype(np.float32)


def dev(x, dt=None):
    t = torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    return t.to(dt) if dt is not None else t


def q16(x, td):
    """fp32 numpy -> (device tensor of the build's 16-bit type, the rounded values as fp32 numpy: what the kernel sees)."""
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(td)
    return t.to(DEV), t.float().numpy()


def host(t):
    return t.float().cpu().numpy().astype(np.float64)


def site(p, kind, layer=LAYER, call=CALL):
    """p = 0: a site that switches the mask off (the eval kernel, bit for bit)."""
    return T.Dropout(SEED, int(kind) | (layer << 8), call, float(p))


@functools.lru_cache(maxsize=None)
def probs_mask(p, N, A, L, call=CALL):
    if p == 0.0:
        return np.ones((N, A, L, L), np.float32)
    return DO.probs_mask(p, SEED, DO.site_id(DO.KIND_PROB, LAYER), call, N, A, L)


@functools.lru_cache(maxsize=None)
def rows_mask(p, kind, layer, rows, cols):
    if p == 0.0:
        return np.ones((rows, cols), np.float32)
    return DO.rows_mask(p, SEED, DO.site_id(kind, layer), CALL, rows, cols)


def check(what, got, want, rtol, atol):
    """|got - want| <= atol + rtol |want| (numpy's assert_allclose), printing the largest error and the worst error / bound."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    err = np.abs(got - want)
    bound = atol + rtol * np.abs(want)
    worst = float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0
    print("[dropout-kernels] %s: max|err| %.3e, worst err / bound %.3f" % (what, float(err.max()) if err.size else 0.0, worst))
    assert np.isfinite(got).all(), what
    assert (err <= bound).all(), "%s: %d of %d elements over the bound, worst err / bound %.3f" % (what, int((err > bound).sum()), err.size, worst)


# ------------------------------------------------------------------------------------------------ attention
def _pitch(kind, L):
    return 32 if kind == "l32" else (L + 31) // 32 * 32


def _rel_table(w, kind, L, A):
    relt = torch.zeros((A, _pitch(kind, L), _pitch(kind, L)), device=DEV)
    T.call("tnr_relpos_table", dev(w), A, L, relt)
    return relt


def _run_attn(kind, sfx, td, qkv, madd, relt, dctx, N, L, A, st):
    """forward + backward through the *_do entry points -> (ctx, lse or None, dqkv, bias_part or None)."""
    Lp = _pitch(kind, L)
    ctx = torch.zeros((N * L, A * D), device=DEV, dtype=td)
    dqkv = torch.zeros((N * L, 3 * A * D), device=DEV, dtype=td)
    if kind == "l32":
        lse, bpart = None, torch.zeros((N, 3 * A * D), device=DEV)
        T.call("tnr_attn_l32_fwd_do" + sfx, qkv, madd, relt, ctx, N, L, A, st)
        T.call("tnr_attn_l32_bwd_do" + sfx, qkv, madd, relt, dctx, dqkv, bpart, N, L, A, st)
    else:
        lse, delta, bpart = torch.zeros((N, A, Lp), device=DEV), torch.zeros((N, A, Lp), device=DEV), None
        T.call("tnr_attn_long_fwd_do" + sfx, qkv, madd, relt, ctx, lse, N, L, A, st)
        T.call("tnr_attn_long_bwd_do" + sfx, qkv, madd, relt, ctx, dctx, lse, delta, dqkv, N, L, A, st)
    torch.cuda.synchronize()
    return ctx, lse, dqkv, bpart


def _onehot(N, L, A, w):
    """(N L, A 64): row r of every sequence holds e_(r - 64 w) in every head's 64 columns for r in window w, zeros elsewhere."""
    x = np.zeros((N, L, A, D), np.float32)
    for r in range(64 * w, min(L, 64 * w + 64)):
        x[:, r, :, r - 64 * w] = 1.0
    return x.reshape(N * L, A * D)


def _by_query(t, N, L, A):
    """(N, A, queries, c) -> the layout of a per-query output (N, queries, A, c)."""
    return t.transpose(0, 2, 1, 3)


def _by_key(t, N, L, A):
    """(N, A, c, keys) -> the layout of a per-key output (N, keys, A, c)."""
    return t.transpose(0, 3, 1, 2)


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("kind,N,L,A", ATTN_CASES)
def test_attention_applied_mask_read_back(kind, N, L, A, dtype, p):
    """q, k and the rel-pos weight at scale 0.1, no padding: every probability is near 1 / L and every kept one is >= 2^-12 (asserted on
    the float64 reference, so that a 16-bit flush cannot produce a false zero).  Per 64-wide window: ctx and dv are exact zeros
    where the oracle mask is 0 and non-zero where it is not, and equal (P o m) within the forward bound; dq (K one-hot) and dk (Q
    one-hot) equal dS / 8 within the backward bound relative to max |dS| / 8, so one flipped mask element shows as an error of that
    element's own size (dS is not zero where an element is dropped: it is -P delta there).

    (1, 1, 1) is the regression case of attn_bwd_kernel's dS for dk: with one key dS is identically 0 and so is the bound; the kernel
    used to return dk = -2.6e-8 in bf16 at p = 0.1, the rounding residue of dP m that a fused multiply-add kept and delta's rounded
    copy of the product did not."""
    td, sfx = BUILDS[dtype]
    tol_f, tol_b = [t / (1.0 - p) for t in ATTN_TOL[kind][dtype]]
    Lp = _pitch(kind, L)
    _, q = q16(rnd((N * L, A * D), 1, 0.1), td)
    _, k = q16(rnd((N * L, A * D), 2, 0.1), td)
    _, v = q16(rnd((N * L, A * D), 3), td)
    dctx_d, dctx = q16(rnd((N * L, A * D), 4), td)
    w = rnd((A, 32), 5, 0.1)
    rel = O.relpos_bias_table(w, L)
    relt = _rel_table(w, kind, L, A)
    madd = np.full((N, Lp), -1e30, np.float32)
    madd[:, :L] = 0.0
    madd_d, zero_add = dev(madd), np.zeros((N, L))
    m = probs_mask(p, N, A, L).astype(np.float64)
    st = site(p, T.DROP_PROB)
    tag = "%s %s p=%.1f (%d,%d,%d)" % (kind, dtype, p, N, L, A)
    for w_ in range((L + 63) // 64):
        lo, hi = 64 * w_, min(L, 64 * w_ + 64)
        hot = _onehot(N, L, A, w_)
        hot_d = dev(hot, td)
        # ---- V one-hot, dctx one-hot: the applied mask in ctx (per-query accessor) and in dv (per-key accessor)
        qkv = np.concatenate([q, k, hot], 1)
        c = R.attn_fwd(qkv, zero_add, rel, N, L, A, m=m)
        pm = c["p"] * m
        assert (pm[m > 0] >= 2.0 ** -12).all()                             # a condition on the inputs
        ctx, _, dqkv, _ = _run_attn(kind, sfx, td, dev(qkv, td), madd_d, relt, hot_d, N, L, A, st)
        got = host(ctx).reshape(N, L, A, D)
        dropped = _by_query(m[:, :, :, lo:hi], N, L, A) == 0
        assert np.array_equal(got[..., :hi - lo] == 0, dropped), (tag, w_, "ctx zero pattern")
        assert (got[..., hi - lo:] == 0).all()
        check("%s w=%d ctx = P o m" % (tag, w_), got[..., :hi - lo], _by_query(pm[:, :, :, lo:hi], N, L, A), tol_f, tol_f)
        got_d = host(dqkv)
        got = got_d[:, 2 * A * D:].reshape(N, L, A, D)
        dropped = _by_key(m[:, :, lo:hi, :], N, L, A) == 0
        assert np.array_equal(got[..., :hi - lo] == 0, dropped), (tag, w_, "dv zero pattern")
        assert (got[..., hi - lo:] == 0).all()
        check("%s w=%d dv = (P o m)^T" % (tag, w_), got[..., :hi - lo], _by_key(pm[:, :, lo:hi, :], N, L, A), tol_f, tol_f)
        want_d, _ = R.attn_bwd(c, hot)
        check("%s w=%d dqkv (one-hot V, dctx)" % (tag, w_), got_d, want_d, tol_b, tol_b * np.abs(want_d).max())
        # ---- K one-hot: dq = dS[:, window] / 8 (the dQ kernel) ; Q one-hot: dk = dS[window, :]^T / 8 (the key-tile kernel)
        for name, qkv, sl, pick in (("dq = dS / 8 (one-hot K)", np.concatenate([q, hot, v], 1), slice(0, A * D),
                                     lambda ds: _by_query(ds[:, :, :, lo:hi], N, L, A)),
                                    ("dk = dS^T / 8 (one-hot Q)", np.concatenate([hot, k, v], 1), slice(A * D, 2 * A * D),
                                     lambda ds: _by_key(ds[:, :, lo:hi, :], N, L, A))):
            c = R.attn_fwd(qkv, zero_add, rel, N, L, A, m=m)
            _, ds = R.attn_bwd(c, dctx)
            _, _, dqkv, _ = _run_attn(kind, sfx, td, dev(qkv, td), madd_d, relt, dctx_d, N, L, A, st)
            got = host(dqkv)[:, sl].reshape(N, L, A, D)
            scale = np.abs(ds).max() / 8.0
            check("%s w=%d %s" % (tag, w_, name), got[..., :hi - lo], pick(ds) / 8.0, tol_b, tol_b * scale)
            assert (np.abs(got[..., hi - lo:]) <= tol_b * scale).all()


def _padding(kind, N, L):
    """The padding masks of test_attention_fwd_bwd (an all-pad sequence) / test_attention_long_fwd_bwd (a half-padded one)."""
    rs = np.random.RandomState(N * 100 + L if kind == "l32" else L)
    mask = (rs.rand(N, L) > 0.3).astype(np.float32)
    mask[0, :] = 1
    if N > 1:
        if kind == "l32":
            mask[1, :] = 0
        else:
            mask[1, L // 2:] = 0
    return mask


@pytest.mark.parametrize("p", [0.0, 0.1, 0.5])
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("kind,N,L,A", ATTN_CASES)
def test_attention_with_dropout_matches_float64(kind, N, L, A, dtype, p):
    """Random qkv at scale 1 under the eval tests' padding masks, mask_add and the rel table through their own kernels: ctx, lse
    (long), all of dqkv and (l32) the fused bias partials against float64; a second forward + backward with the same site is
    bit-identical; a site that differs only in its forward-call number changes ctx exactly when it changes the reference."""
    td, sfx = BUILDS[dtype]
    tol_f0, _ = ATTN_TOL[kind][dtype]
    tol_f, tol_b = [t / (1.0 - p) for t in ATTN_TOL[kind][dtype]]
    Lp = _pitch(kind, L)
    qkv_d, qkv = q16(rnd((N * L, 3 * A * D), 1), td)
    dctx_d, dctx = q16(rnd((N * L, A * D), 3), td)
    mask = _padding(kind, N, L)
    w = rnd((A, 32), 2, 0.5)
    rel = O.relpos_bias_table(w, L)
    relt = _rel_table(w, kind, L, A)
    H = 768
    tok = np.concatenate([np.ones((N, L)), mask], 1).astype(np.int64)
    madd = torch.zeros((N, Lp), device=DEV)
    z = torch.zeros((600, H), device=DEV)
    T.call("tnr_embed_ln_fwd" + sfx, dev(tok), N, L, H, z, z, z[0], z[0], z[0], 1e-12, torch.zeros((N * L, H), device=DEV, dtype=td), madd)
    torch.cuda.synchronize()
    mask_add = (1.0 - mask) * -10000.0
    assert np.array_equal(madd.cpu().numpy()[:, :L], mask_add.astype(np.float32)) and (madd.cpu().numpy()[:, L:] <= -1e29).all()
    assert np.array_equal(relt.cpu().numpy()[:, :L, :L], rel)
    st = site(p, T.DROP_PROB)
    tag = "%s %s p=%.1f (%d,%d,%d)" % (kind, dtype, p, N, L, A)
    ctx, lse, dqkv, bpart = _run_attn(kind, sfx, td, qkv_d, madd, relt, dctx_d, N, L, A, st)
    c = R.attn_fwd(qkv, mask_add, rel, N, L, A, m=probs_mask(p, N, A, L))
    check(tag + " ctx", host(ctx), c["ctx"], tol_f, tol_f)
    if lse is not None:
        check(tag + " lse", host(lse)[:, :, :L], c["lse"], 1e-3, tol_f0)                   # the mask does not touch it
    want_d, _ = R.attn_bwd(c, dctx)
    got = host(dqkv)
    scale = np.abs(want_d).max()
    check(tag + " dqkv", got, want_d, tol_b, tol_b * scale)
    if bpart is not None:
        check(tag + " bias partials", host(bpart).sum(0), got.sum(0), 1e-3, 1e-3 * scale * N * L)
    again = _run_attn(kind, sfx, td, qkv_d, madd, relt, dctx_d, N, L, A, st)
    for a_, b_ in zip((ctx, lse, dqkv, bpart), again):
        assert a_ is None or torch.equal(a_, b_), tag
    other, _, _, _ = _run_attn(kind, sfx, td, qkv_d, madd, relt, dctx_d, N, L, A, site(p, T.DROP_PROB, call=CALL + 1))
    c2 = R.attn_fwd(qkv, mask_add, rel, N, L, A, m=probs_mask(p, N, A, L, CALL + 1))
    assert (not torch.equal(other, ctx)) == bool((c2["ctx"] != c["ctx"]).any()), tag
    if N * A * L * L >= 64:
        assert p == 0.0 or not torch.equal(other, ctx), tag


# ------------------------------------------------------------------------------------------------ GEMM
# the option sets of tests/test_dropout_split_gpu.py
ROUTES = {"128x128": {"ver": 1}, "256x128": {"ver": 2, "allow_fine": 0}, "224x256": {"bm": 224, "allow_fine": 0},
          "256x256": {"bm": 256, "allow_fine": 0}}
DEFAULTS = {"ver": 3, "bm": 0, "allow_fine": 1}
ROUTE_ID = {"128x128": T.ROUTE_128, "256x128": T.ROUTE_256x128, "224x256": T.ROUTE_224, "256x256": T.ROUTE_256}
GEMM_M = {"128x128": (1, 129), "256x128": (129, 257), "224x256": (129, 225), "256x256": (129, 257)}


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("route", list(ROUTES))
def test_gemm_with_a_site_matches_float64_on_every_route(dtype, route):
    """tnr_gemm_nt_do against (A B^T + bias) o m + res with the oracle's rows mask (element m N + n), K = 128, N in {256, 768}, sites
    DROP_ATTN_OUT and DROP_FFN_OUT at p = 0.1 (and p = 0: the rounding floor), flags EPI_BIAS | EPI_RES without column sums (the one
    set engine.py passes with a site) and EPI_BIAS alone.
    M: the smallest that yields the route under its pinned options - 1 for the 128x128 kernel (any M takes it under ver = 1), 129 for
    the three others (M <= 128 always takes the 128x128 kernel) - none a multiple of the route's row tile, plus one row past the
    first row tile (129 / 257 / 225 / 257) so that a second, ragged tile runs.
    Where the mask is 0, C == res bit for bit (EPI_BIAS alone: C == 0); rows >= M of an over-allocated C stay untouched."""
    td, sfx = BUILDS[dtype]
    L_ = T.lib()
    K, pad = 128, 8
    try:
        for k_, v_ in ROUTES[route].items():
            assert L_.tnr_gemm_set_option(k_.encode(), v_) == 0
        for N in (256, 768):
            b_d, b = q16(rnd((N, K), 2, 0.1), td)
            bias = rnd((N,), 3)
            for M in GEMM_M[route]:
                a_d, a = q16(rnd((M, K), 1), td)
                r_d, r = q16(rnd((M, N), 4), td)
                for flags in (T.EPI_BIAS | T.EPI_RES, T.EPI_BIAS):
                    assert T.query("tnr_gemm_nt_route" + sfx, M, N, K, flags) == ROUTE_ID[route]
                    for kind in (T.DROP_ATTN_OUT, T.DROP_FFN_OUT):
                        for p in (0.0, 0.1):
                            m = rows_mask(p, kind, LAYER, M, N)
                            c = torch.full((M + pad, N), 5.0, device=DEV, dtype=td)
                            res = r_d if flags & T.EPI_RES else None
                            T.call("tnr_gemm_nt_do" + sfx, a_d, K, b_d, K, c, N, M, N, K, dev(bias), res, N if res is not None else 0,
                                   None, 0, flags, None, site(p, kind))
                            torch.cuda.synchronize()
                            assert (c[M:].float() == 5.0).all(), (route, M, N, "rows past M")
                            got = host(c[:M])
                            want = R.linear_do(a, b, bias, m=m, res=r if res is not None else None)
                            assert np.array_equal(got[m == 0], (r.astype(np.float64) if res is not None else np.zeros_like(got))[m == 0])
                            tag = "gemm %s %s M=%d N=%d flags=%d site=%d p=%.1f" % (route, dtype, M, N, flags, kind, p)
                            check(tag, got[m != 0], want[m != 0], GEMM_RTOL / (1.0 - p), GEMM_ATOL / (1.0 - p))
    finally:
        for k_, v_ in DEFAULTS.items():
            L_.tnr_gemm_set_option(k_.encode(), v_)


# ------------------------------------------------------------------------------------------------ embeddings
PAD = 1                                         # RoBERTa's padding_idx


@pytest.mark.parametrize("case", ["site", "pos_ids", "both"])
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("N,L,H", [(37, 30, 768), (3, 200, 256)])
def test_embeddings_with_a_site_and_pos_ids(N, L, H, dtype, case):
    """tnr_embed_ln_fwd_do and tnr_embed_ln_fwd_indexed_do with a site only, a pos_ids table only (drop NULL: what the engine issues
    for RoBERTa in eval) and both.  pos_ids: RoBERTa's own - cumulative non-pad count + padding_idx - with an all-pad row; the
    position table has L + padding_idx + 1 rows.  out == 0 exactly where the oracle's (N L, H) mask is 0, the rest against float64;
    mask_add is what the plain entry point writes; the indexed variant equals the direct one bit for bit on the gathered rows."""
    td, sfx = BUILDS[dtype]
    p = 0.0 if case == "pos_ids" else 0.1
    tol = EMB_TOL[dtype] / (1.0 - p)
    V, n_rows = 500, N + 6
    rs = np.random.RandomState(N + L)
    ids_t = rs.randint(2, V, (n_rows, L))
    keep = rs.rand(n_rows, L) > 0.3
    keep[0], keep[3] = True, False               # a full row, an all-pad row
    ids_t[~keep] = PAD
    nidx = rs.randint(0, n_rows, N).astype(np.int32)
    nidx[:3] = (3, n_rows - 1, 0)                # the all-pad row, the table's last row, a full row
    ids, mask = ids_t[nidx], keep[nidx].astype(np.int64)
    pid_t = R.roberta_pos_ids(ids_t, PAD).astype(np.int32)
    assert pid_t.max() <= L + PAD and (pid_t[3] == PAD).all()
    word, pos, type0 = rnd((V, H), 1), rnd((L + PAD + 1, H), 2), rnd((H,), 3)
    gamma, beta = 1 + rnd((H,), 4, 0.1), rnd((H,), 5, 0.1)
    emb = [dev(x) for x in (word, pos, type0, gamma, beta)]
    use_pos = case != "site"
    st = None if case == "pos_ids" else site(p, T.DROP_EMB, layer=0)
    Lp = (L + 31) // 32 * 32
    new = lambda: (torch.full((N * L, H), 9.0, device=DEV, dtype=td), torch.full((N, Lp), 9.0, device=DEV))
    # direct: the gathered rows as an int64 [ids | mask] table, pos_ids laid out like it
    tok = dev(np.concatenate([ids, mask], 1).astype(np.int64))
    out, madd = new()
    T.call("tnr_embed_ln_fwd_do" + sfx, tok, N, L, H, *emb, 1e-12, out, madd, st, dev(pid_t[nidx]) if use_pos else None)
    # indexed: the resident int32 table + news indices, pos_ids laid out like the table
    tab = dev(np.concatenate([ids_t, keep.astype(np.int64)], 1).astype(np.int32))
    out_i, madd_i = new()
    T.call("tnr_embed_ln_fwd_indexed_do" + sfx, tab, dev(nidx), N, L, H, *emb, 1e-12, out_i, madd_i, st, dev(pid_t) if use_pos else None)
    out_p, madd_p = new()
    T.call("tnr_embed_ln_fwd" + sfx, tok, N, L, H, *emb, 1e-12, out_p, madd_p)
    torch.cuda.synchronize()
    assert torch.equal(out_i, out) and torch.equal(madd_i, madd) and torch.equal(madd, madd_p)
    ma = madd.cpu().numpy()
    assert np.array_equal(ma[:, :L], ((1.0 - mask) * -10000.0).astype(np.float32)) and (ma[:, L:] <= -1e29).all()
    m = rows_mask(p, DO.KIND_EMB, 0, N * L, H)
    want = R.embed_ln(ids, word, pos, type0, gamma, beta, 1e-12, m=m, pos_ids=pid_t[nidx] if use_pos else None)
    got = host(out)
    assert (got[m == 0] == 0).all()
    if p > 0:
        assert 0.08 < (m == 0).mean() < 0.12
    check("embeddings %s %s (%d,%d,%d)" % (case, dtype, N, L, H), got[m != 0], want[m != 0], tol, tol)
