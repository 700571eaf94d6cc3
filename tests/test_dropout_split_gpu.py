"""Dropout sites split at a row (stage 1's joint passes: the body pass's token rows directly behind the title pass's, one launch
over both).  tnr_gemm_nt_do_split / tnr_ln_bwd_do_split over M rows must give exactly what the two per-pass _do calls give - the
head site on rows [0, split), the tail site on rows [split, M) with the row index counted from split - on every GEMM route that
takes a dropout site, at splits on and off tile boundaries (4 800 = N Lt at 30 / 128 lies inside a tile), in both dtypes."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import tnr_hip as T                            # noqa: E402
from oracle import dropout_oracle as DO       # noqa: E402

DEV = "cuda:0"
SEED, P = 0x5EED0001, 0.1
M_JOINT = 4800 + 4096                         # 30 / 128, B = 32: 160 titles x 30 + 32 bodies x 128 token rows
SPLITS = (0, 1, 256, 4800, M_JOINT)
DT = {"bf16": torch.bfloat16, "fp16": torch.float16}
# tnr_gemm_set_option settings that pin each route a dropout site can take (every launch of a case, the per-pass references
# included, runs under them); the defaults are restored behind every case
ROUTES = {"128x128": {"ver": 1}, "256x128": {"ver": 2, "allow_fine": 0}, "224x256": {"bm": 224, "allow_fine": 0},
          "256x256": {"bm": 256, "allow_fine": 0}}
DEFAULTS = {"ver": 3, "bm": 0, "allow_fine": 1}


def _name(n, dtype):
    return n + ("_f16" if dtype == "fp16" else "")


def _sites(kind, layer=1):
    head = T.Dropout.site_of(P, SEED, kind, layer, 6)        # forward call 2 * 3 + 0: the title pass of step 3
    tail = T.Dropout.site_of(P, SEED, kind, layer, 7)        # ... and its body pass
    return head, tail


def _rand(shape, dtype, g, scale=1.0):
    return (torch.randn(shape, generator=g) * scale).to(DT[dtype]).to(DEV)


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("route", list(ROUTES))
def test_gemm_split_site_equals_the_two_per_pass_launches(dtype, route):
    """attention-output Linear of the joint passes (K = H = 768, bias + dropout + residual): C over M rows with the split site ==
    C of rows [0, split) under the head site ++ C of rows [split, M) under the tail site, bit for bit; a NULL tail or split = M is
    the plain _do call."""
    L = T.lib()
    M, N, K = M_JOINT, 768, 768
    g = torch.Generator().manual_seed(5)
    A, W, R = _rand((M, K), dtype, g), _rand((N, K), dtype, g, 0.04), _rand((M, N), dtype, g)
    bias = (torch.randn(N, generator=g) * 0.1).to(DEV)
    head, tail = _sites(T.DROP_ATTN_OUT)
    flags = T.EPI_BIAS | T.EPI_RES
    nt = _name("tnr_gemm_nt_do", dtype)
    ns = _name("tnr_gemm_nt_do_split", dtype)

    def run(a, r, c, m, d):
        T.call(nt, a, K, W, K, c, N, m, N, K, bias, r, N, None, 0, flags, None, d)

    try:
        for k, v in ROUTES[route].items():
            assert L.tnr_gemm_set_option(k.encode(), v) == 0
        want = {"128x128": T.ROUTE_128, "256x128": T.ROUTE_256x128, "224x256": T.ROUTE_224, "256x256": T.ROUTE_256}[route]
        assert T.query(_name("tnr_gemm_nt_route", dtype), M, N, K, flags) == want
        for split in SPLITS:
            ref = torch.full((M, N), float("nan"), device=DEV, dtype=DT[dtype])
            if split > 0:
                run(A[:split], R[:split], ref[:split], split, head)
            if split < M:
                run(A[split:], R[split:], ref[split:], M - split, tail)
            got = torch.full_like(ref, float("nan"))
            T.call(ns, A, K, W, K, got, N, M, N, K, bias, R, N, None, 0, flags, None, head, tail, split)
            torch.cuda.synchronize()
            assert torch.equal(got, ref), (route, dtype, split)
        # no tail / split = M: the _do call itself
        plain = torch.empty((M, N), device=DEV, dtype=DT[dtype])
        run(A, R, plain, M, head)
        for tl, sp in ((None, 4800), (tail, M)):
            got = torch.full_like(plain, float("nan"))
            T.call(ns, A, K, W, K, got, N, M, N, K, bias, R, N, None, 0, flags, None, head, tl, sp)
            torch.cuda.synchronize()
            assert torch.equal(got, plain), (route, dtype, sp)
    finally:
        for k, v in DEFAULTS.items():
            L.tnr_gemm_set_option(k.encode(), v)


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_gemm_split_site_ffn_output_shape(dtype):
    """The FFN-output Linear (K = 3 072) at the default route of the joint M, split at N Lt."""
    M, N, K, split = M_JOINT, 768, 3072, 4800
    g = torch.Generator().manual_seed(6)
    A, W, R = _rand((M, K), dtype, g), _rand((N, K), dtype, g, 0.02), _rand((M, N), dtype, g)
    bias = (torch.randn(N, generator=g) * 0.1).to(DEV)
    head, tail = _sites(T.DROP_FFN_OUT, 0)
    flags = T.EPI_BIAS | T.EPI_RES
    nt = _name("tnr_gemm_nt_do", dtype)
    ref = torch.full((M, N), float("nan"), device=DEV, dtype=DT[dtype])
    T.call(nt, A[:split], K, W, K, ref[:split], N, split, N, K, bias, R[:split], N, None, 0, flags, None, head)
    T.call(nt, A[split:], K, W, K, ref[split:], N, M - split, N, K, bias, R[split:], N, None, 0, flags, None, tail)
    got = torch.full_like(ref, float("nan"))
    T.call(_name("tnr_gemm_nt_do_split", dtype), A, K, W, K, got, N, M, N, K, bias, R, N, None, 0, flags, None, head, tail, split)
    torch.cuda.synchronize()
    assert torch.equal(got, ref)


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_ln_bwd_split_site_equals_the_two_per_pass_calls(dtype):
    """LayerNorm backward behind the split Linear: dx and dxm bit for bit against the two per-pass calls; the reduced dgamma /
    dbeta / dxsum are the same row sums in another grouping (fp32 reordering)."""
    M, H = M_JOINT, 768
    g = torch.Generator().manual_seed(7)
    x, dy = _rand((M, H), dtype, g), _rand((M, H), dtype, g, 0.1)
    gamma = (1.0 + 0.1 * torch.randn(H, generator=g)).to(DEV)
    beta = (0.1 * torch.randn(H, generator=g)).to(DEV)
    y = torch.empty_like(x)
    stats = torch.empty((M, 2), device=DEV)
    T.call(_name("tnr_ln_fwd", dtype), x, gamma, beta, 1e-12, y, stats, M, H)
    part = torch.empty(T.query("tnr_ln_bwd_part_elems", M, H), device=DEV)
    head, tail = _sites(T.DROP_FFN_OUT)
    nd, ns = _name("tnr_ln_bwd_do", dtype), _name("tnr_ln_bwd_do_split", dtype)

    def sums():
        return [torch.zeros(H, device=DEV) for _ in range(3)]

    for split in SPLITS:
        dx_r, dxm_r = torch.full_like(x, float("nan")), torch.full_like(x, float("nan"))
        red_r = [torch.zeros(H, device=DEV, dtype=torch.float64) for _ in range(3)]
        for lo, hi, d in ((0, split, head), (split, M, tail)):
            if hi > lo:
                o = sums()
                T.call(nd, dy[lo:hi], x[lo:hi], stats[lo:hi], gamma, dx_r[lo:hi], o[0], o[1], o[2], part, hi - lo, H, dxm_r[lo:hi], d)
                for a, b in zip(red_r, o):
                    a += b.double()
        dx, dxm = torch.full_like(x, float("nan")), torch.full_like(x, float("nan"))
        red = sums()
        T.call(ns, dy, x, stats, gamma, dx, red[0], red[1], red[2], part, M, H, dxm, head, tail, split)
        torch.cuda.synchronize()
        assert torch.equal(dx, dx_r) and torch.equal(dxm, dxm_r), (dtype, split)
        for a, b in zip(red, red_r):
            assert float((a.double() - b).norm()) <= 1e-5 * float(b.norm()) + 1e-6, (dtype, split)
    # no tail / split = M: the _do call itself
    dx_p, dxm_p = torch.empty_like(x), torch.empty_like(x)
    T.call(nd, dy, x, stats, gamma, dx_p, None, None, None, part, M, H, dxm_p, head)
    for tl, sp in ((None, 4800), (tail, M)):
        dx, dxm = torch.full_like(x, float("nan")), torch.full_like(x, float("nan"))
        T.call(ns, dy, x, stats, gamma, dx, None, None, None, part, M, H, dxm, head, tl, sp)
        torch.cuda.synchronize()
        assert torch.equal(dx, dx_p) and torch.equal(dxm, dxm_p), sp


def test_split_mask_dump_is_two_oracle_sites():
    """tnr_dropout_mask_split == oracle/dropout_oracle.py's rows mask of the head site on [0, split) followed by the tail site's
    on [split, rows), each counted from its own first row."""
    for (p, seed, kind, layer, calls, rows, cols, split) in ((0.1, 777, DO.KIND_FFN_OUT, 1, (4, 5), 1000, 768, 600),
                                                             (0.25, 2 ** 40 + 5, DO.KIND_ATTN_OUT, 0, (10, 11), 333, 256, 1),
                                                             (0.1, 1, DO.KIND_ATTN_OUT, 11, (0, 2 ** 31 + 1), 64, 3072, 63)):
        head = T.Dropout.site_of(p, seed, kind, layer, calls[0])
        tail = T.Dropout.site_of(p, seed, kind, layer, calls[1])
        out = torch.full((rows, cols), -1.0, device=DEV)
        T.call("tnr_dropout_mask_split", head, tail, split, rows, cols, out)
        sid = DO.site_id(kind, layer)
        want = np.concatenate([DO.rows_mask(p, seed, sid, calls[0], split, cols),
                               DO.rows_mask(p, seed, sid, calls[1], rows - split, cols)])
        assert np.array_equal(out.cpu().numpy(), want), (rows, split)
        # no tail: tnr_dropout_mask itself
        plain = torch.empty((rows, cols), device=DEV)
        T.call("tnr_dropout_mask", head, rows, cols, plain)
        T.call("tnr_dropout_mask_split", head, None, split, rows, cols, out)
        assert torch.equal(out, plain)


def test_split_sites_that_disagree_are_refused():
    x = torch.zeros((64, 768), device=DEV, dtype=torch.bfloat16)
    w = torch.zeros((768, 768), device=DEV, dtype=torch.bfloat16)
    head, tail = _sites(T.DROP_ATTN_OUT)
    bad = [T.Dropout(tail.seed + 1, tail.site, tail.call, tail.p), T.Dropout(tail.seed, tail.site + 1, tail.call, tail.p),
           T.Dropout(tail.seed, tail.site, tail.call, 0.2)]
    for t_ in bad:
        with pytest.raises(T.TnrError, match="share seed, site and p"):
            T.call("tnr_gemm_nt_do_split", x, 768, w, 768, x, 768, 64, 768, 768, None, None, 0, None, 0, 0, None, head, t_, 32)
    for sp in (-1, 65):
        with pytest.raises(T.TnrError, match="split row"):
            T.call("tnr_gemm_nt_do_split", x, 768, w, 768, x, 768, 64, 768, 768, None, None, 0, None, 0, 0, None, head, tail, sp)
