"""tests/gemm_ref.py (the float64 references and bounds of tests/test_gemm_kernels_gpu.py) against oracle/newsrec_oracle.py, which
tests/test_oracle_golden.py pins to the reference implementation: GELU, GELU', and the Linear forward / backward of the FFN and of
the attention output on a tiny layer.  The tilings the GPU file pins are asserted here with the library's host-only
tnr_gemm_nt_plan, and the error of the erf approximation that fills the GELU tables is measured on the restatement of erf_as.

Bound: the oracle computes in fp32, the helpers in float64 -> rtol 1e-5, plus 1e-5 of the tensor's largest magnitude (an fp32 sum's
rounding error is relative to its terms, not to a result that cancels)."""
import ctypes
import math

import numpy as np
import pytest

import gemm_ref as R
import tnr_hip as T
from oracle import newsrec_oracle as O

N, L, H, A, I, LAYER = 3, 11, 64, 4, 256, 1
RTOL = 1e-5


def close(got, want, what):
    want = np.asarray(want, np.float64)
    np.testing.assert_allclose(got, want, rtol=RTOL, atol=RTOL * np.abs(want).max(), err_msg=what)


def test_flags_are_the_headers():
    for name in ("BIAS", "GELU", "TANH", "RES", "MULDGELU", "OUTF32", "AUXOUT", "COLSUM"):
        assert getattr(R, "EPI_" + name) == getattr(T, "EPI_" + name), name
    assert R.EPI_DROPOUT == 256


def test_gelu_and_its_derivative_equal_the_oracle():
    x = np.concatenate([np.linspace(-9, 9, 2001), np.random.RandomState(0).standard_normal(1000) * 3]).astype(np.float32)
    close(R.gelu(x), O.gelu(x), "gelu")
    close(R.gelu_grad(x), O.gelu_grad(x), "gelu_grad")
    # the derivative is the derivative: central differences in float64
    xs = np.linspace(-6, 6, 1201)
    h = 1e-5
    np.testing.assert_allclose(R.gelu_grad(xs), (R.gelu(xs + h) - R.gelu(xs - h)) / (2 * h), rtol=0, atol=1e-9)
    assert abs(R.GELU_SLOPE - R._sup(R.gelu_grad)) < 1e-9


@pytest.fixture(scope="module")
def layer():
    rs = np.random.RandomState(11)
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
    x = rs.standard_normal((N, L, H)).astype(np.float32)
    mask = (rs.rand(N, L) > 0.3).astype(np.float32)
    mask[0] = 1
    mask_add = ((1.0 - mask) * -10000.0).astype(np.float32)
    rel = O.relpos_bias_table((rs.standard_normal((A, 32)) * 0.5).astype(np.float32), L)
    dy = rs.standard_normal((N, L, H)).astype(np.float32)
    y, c = O.bert_layer_fwd(P, LAYER, x, mask_add, rel, A)
    _, G = O.bert_layer_bwd(P, LAYER, dy, c, A)
    return P, x, dy, c, G


def test_linear_forward_equals_the_oracles_ffn_and_attention_output(layer):
    """BertIntermediate = EPI_BIAS | EPI_GELU (| EPI_AUXOUT: the pre-activation u), BertSelfOutput / BertOutput = EPI_BIAS | EPI_RES
    in front of their LayerNorms."""
    P, x, dy, c, G = layer
    p = O._lp(LAYER)
    M = N * L
    x2, ctx, h1 = x.reshape(M, H), c["ctx"].reshape(M, H), c["h1"].reshape(M, H)
    ao, _ = R.linear(ctx, P[p + "attention.output.dense.weight"], P[p + "attention.output.dense.bias"], res=x2, flags=R.EPI_BIAS | R.EPI_RES)
    close(ao, O.linear(ctx, P[p + "attention.output.dense.weight"], P[p + "attention.output.dense.bias"]) + x2, "attention output + residual")
    h1_ref, _ = O.layer_norm_fwd(ao.astype(np.float32).reshape(N, L, H), P[p + "attention.output.LayerNorm.weight"],
                                 P[p + "attention.output.LayerNorm.bias"], 1e-12)
    close(h1_ref, c["h1"], "h1 through the helper")
    g, u = R.linear(h1, P[p + "intermediate.dense.weight"], P[p + "intermediate.dense.bias"], flags=R.EPI_BIAS | R.EPI_GELU)
    close(u, c["u"].reshape(M, I), "FFN pre-activation")
    close(g, c["g"].reshape(M, I), "FFN activation")
    f, _ = R.linear(g, P[p + "output.dense.weight"], P[p + "output.dense.bias"], res=h1, flags=R.EPI_BIAS | R.EPI_RES)
    close(f, O.linear(c["g"].reshape(M, I), P[p + "output.dense.weight"], P[p + "output.dense.bias"]) + h1, "FFN output + residual")
    t, pre = R.linear(h1, P[p + "intermediate.dense.weight"][:16], P[p + "intermediate.dense.bias"][:16], flags=R.EPI_BIAS | R.EPI_TANH)
    close(t, np.tanh(O.linear(h1, P[p + "intermediate.dense.weight"][:16], P[p + "intermediate.dense.bias"][:16])), "tanh(fc1)")
    plain, pre0 = R.linear(h1, P[p + "intermediate.dense.weight"])
    assert plain is pre0 or np.array_equal(plain, pre0)


def test_linear_backward_equals_the_oracles_ffn_and_attention_output(layer):
    """The dgrads as the engine issues them (B = the transposed weight): FFN down -> EPI_MULDGELU (| EPI_COLSUM: the bias gradient),
    FFN up -> EPI_RES with the residual branch's gradient; the weight gradients dY^T X; the bias gradients = column sums."""
    P, x, dy, c, G = layer
    p = O._lp(LAYER)
    M = N * L
    r2 = lambda t: np.asarray(t).reshape(M, -1)
    dypre, _, _ = O.layer_norm_bwd(dy, c["ln2"], P[p + "output.LayerNorm.weight"])
    w2, w1 = P[p + "output.dense.weight"], P[p + "intermediate.dense.weight"]
    du, dgact = R.linear(r2(dypre), w2.T, aux=r2(c["u"]), flags=R.EPI_MULDGELU)
    close(dgact, r2(dypre) @ w2, "dgrad of the FFN output")
    close(du, (r2(dypre) @ w2) * O.gelu_grad(r2(c["u"])), "... times GELU'(u)")
    dx_, dw_, db_ = R.linear_bwd(r2(dypre), r2(c["g"]), w2)
    close(dx_, dgact, "linear_bwd dx")
    close(dw_, G[p + "output.dense.weight"], "dW of the FFN output")
    close(db_, G[p + "output.dense.bias"], "db of the FFN output")
    close(R.wgrad(du, r2(c["h1"]), M), G[p + "intermediate.dense.weight"], "dW of the FFN input")
    close(du.sum(0), G[p + "intermediate.dense.bias"], "db of the FFN input = column sums of the MULDGELU output")
    dh1, _ = R.linear(du, w1.T, res=r2(dypre), flags=R.EPI_RES)
    dh1pre, _, _ = O.layer_norm_bwd(dh1.astype(np.float32).reshape(N, L, H), c["ln1"], P[p + "attention.output.LayerNorm.weight"])
    close(R.wgrad(r2(dh1pre), r2(c["ctx"]), M), G[p + "attention.output.dense.weight"], "dW of the attention output")
    close(r2(dh1pre).sum(0), G[p + "attention.output.dense.bias"], "db of the attention output")


def test_wgrad_rows_scale_and_accumulate():
    rs = np.random.RandomState(3)
    dy, x = rs.standard_normal((70, 8)).astype(np.float32), rs.standard_normal((70, 12)).astype(np.float32)
    dw0 = rs.standard_normal((8, 12)).astype(np.float32)
    close(R.wgrad(dy, x, 50), dy[:50].T @ x[:50], "rows past M are not part of the sum")
    close(R.wgrad(dy, x, 50, 0.25, dw0), dw0 + np.float32(0.25) * (dy[:50].T @ x[:50]), "out_scale applies to the product only")
    assert (R.wgrad_mag(dy, x, 50, -0.25, dw0) >= np.abs(R.wgrad(dy, x, 50, -0.25, dw0))).all()
    assert R.wgrad_splits(449, 3) == (3, 3, 8) and R.wgrad_splits(449, 5) == (4, 2, 8) and R.wgrad_splits(65, 64) == (2, 1, 2)
    assert R.wgrad_splits(1, 7) == (1, 1, 1) and R.wgrad_splits(200, 3) == (2, 2, 4)


def test_erf_approximation_error_measured():
    """csrc/common.h: erf_as is Abramowitz & Stegun 7.1.26, |error| <= 1.5e-7 in exact arithmetic; its fp32 evaluation (Horner's rule
    with coefficients up to 1.45 that cancel) adds more than that: 5.3e-7 in all.  The table nodes carry half of it (Phi = 0.5 (1 + erf)).
    Measured on the float32 restatement against float64 erf; gemm_ref.table_bound builds on the node errors."""
    z = np.linspace(-6, 6, 200001).astype(np.float32)
    r, _ = R.erf_as(z)
    e_erf = float(np.abs(r.astype(np.float64) - R._erf(z.astype(np.float64))).max())
    e_phi, e_dg = R.lut_node_error(False), R.lut_node_error(True)
    print("[gemm-ref] erf_as max error %.3e ; table nodes: Phi %.3e, GELU' %.3e ; table bounds: Phi %.3e, GELU' %.3e"
          % (e_erf, e_phi, e_dg, R._table_bound(False), R._table_bound(True)))
    # a ceiling for the measurement (a broken restatement would be far outside): A&S's 1.5e-7, Horner's rule in fp32 on p, a
    # polynomial of degree 5 in t <= 1 whose coefficients sum to 4.47 in magnitude (2 n u sum|c_i|), the roundings of p e and 1 - p e
    e_max = 1.5e-7 + (10 * 4.47 + 2) * R.U24
    assert 1e-7 < e_erf <= e_max
    assert e_phi <= 0.5 * e_max + R.U24            # 0.5 (1 + erf): one more rounding of a value <= 1
    assert e_dg <= 0.5 * e_max + 4 * R.U24         # + x e / sqrt(2 pi) (|.| <= 0.25, two roundings) and an addition (<= 1.13)
    # scipy's erf against math.erf: the float64 reference itself
    zz = np.linspace(-6, 6, 2001)
    assert np.abs(R._erf(zz) - np.array([math.erf(t) for t in zz])).max() < 1e-15
    # interpolation term of the bounds: h^2 / 8 max|f''|, 1.85e-6 for Phi (csrc/gemm.hip quotes 1.8e-6)
    assert 1.8e-6 < R._table_bound(False) - e_phi < 2.3e-6
    assert R._table_bound(True) < 8e-6


def _plan(M, Nc, flags, n_cu):
    mi, P, x = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    ref = lambda v: ctypes.cast(ctypes.byref(v), ctypes.c_void_p)
    assert T.lib().tnr_gemm_nt_plan(M, Nc, flags, n_cu, ref(mi), ref(P), ref(x)) == 0
    return mi.value, P.value, x.value


def test_pinned_plans_are_the_librarys():
    """Every (mi, panels, tall) that tests/test_gemm_kernels_gpu.py asserts before a persistent launch, under the options it pins
    ("bm", "allow_fine" = 0, "cus" = 8): host arithmetic only.  The panels cover [0, M) and the two mixed plans have 2 <= tall <=
    panels - 2, M % 32 != 0 and more tiles than workgroups."""
    L_ = T.lib()
    try:
        for (bm, M, Nc), want in sorted(R.PLANS.items()):
            assert L_.tnr_gemm_set_option(b"bm", bm) == 0 and L_.tnr_gemm_set_option(b"allow_fine", 0) == 0
            assert L_.tnr_gemm_set_option(b"cus", R.PLAN_CUS) == 0
            assert _plan(M, Nc, 0, R.PLAN_CUS) == want == R.plan(bm, M, Nc, 0), (bm, M, Nc)
            cs = _plan(M, Nc, R.EPI_MULDGELU | R.EPI_COLSUM, R.PLAN_CUS)
            assert cs == R.plan(bm, M, Nc, R.EPI_COLSUM) == (8, (M + 255) // 256, (M + 255) // 256), (bm, M, Nc)
            rows = R.panel_rows(M, *want)
            assert rows[0][0] == 0 and all(a[0] + a[1] == b[0] for a, b in zip(rows, rows[1:])) and rows[-1][0] + rows[-1][1] >= M
            assert rows[-1][0] < M, "no panel without a live row"
            # the route these options give (no device needed: "cus" stands in for the device's CU count)
            assert T.query("tnr_gemm_nt_route", M, Nc, 128, 0) == bm
            assert T.query("tnr_gemm_nt_route", M, Nc, 128, R.EPI_MULDGELU | R.EPI_COLSUM) == 256
        for bm, M, Nc in ((256, 1153, 768), (224, 993, 768)):
            mi, P, x = R.PLANS[(bm, M, Nc)]
            assert (mi, P, x) == (bm // 32, 5, 2) and 2 <= x <= P - 2 and M % 32 and P * (Nc // 256) > R.PLAN_CUS
    finally:
        for k, v in (("bm", 0), ("allow_fine", 1), ("cus", 0)):
            L_.tnr_gemm_set_option(k.encode(), v)
