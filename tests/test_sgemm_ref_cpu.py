"""tests/sgemm_ref.py judged without a GPU and without the library: the reference against numpy.einsum on strided views, the
written set, the split rule on literal pairs, and the two conditions its bound has to meet on EVERY case of the tables that
tests/test_sgemm_kernels_gpu.py runs - an emulated fp32 fma chain lies inside it (it is not too tight), and every applicable
mutant of sgemm_ref.mutants lies outside it in at least half of the written elements (it is tight enough to see a defect).
EXPERIMENTS.md item 79 records the printed figures."""
import numpy as np
import pytest

import sgemm_ref as R

f32, f64 = np.float32, np.float64


def emulate(c_flat0, p):
    """The chain in fp32: one fma (one rounding) per k in k order, the slices of a split summed in slice order, then alpha, bias
    and beta each rounded on its own."""
    A, B, bias, ci = R.operands(p)
    K = p["K"]
    kchunk, slices = R.effective_split(K, p["ksplit"])
    total = None
    for s in range(slices):
        acc = np.zeros(ci.shape, f32)
        for k in range(s * kchunk, min(K, (s + 1) * kchunk)):
            acc = (acc.astype(f64) + A[:, :, None, k] * B[:, None, :, k]).astype(f32)     # the product of two fp32 is exact in float64
        total = acc if total is None else total + acc
    v = f32(p["alpha"]) * total + bias.astype(f32)[:, None, :]
    out = np.asarray(c_flat0, f32).copy()
    if p["beta"] != 0:
        v = v + f32(p["beta"]) * out[ci]
    assert v.dtype == f32
    out[ci] = v
    return out


@pytest.mark.parametrize("name", R.CASES)
def test_fp32_chain_stays_inside_the_bound(name):
    p, c0 = R.case(name)
    want, bound, written = R.apply(c0, p)
    got = emulate(c0, p).astype(f64)
    assert np.array_equal(got[~written].view(np.int64), want[~written].view(np.int64))
    err = np.abs(got[written] - want[written])
    worst = float((err / bound[written]).max())
    print("[sgemm-ref] %s: emulated chain max|err| %.3e, worst err / bound %.4f" % (name, float(err.max()), worst))
    assert np.isfinite(got[written]).all() and (bound[written] > 0).all()
    assert worst <= 1.0


@pytest.mark.parametrize("name", R.CASES)
def test_every_mutant_leaves_the_bound_in_half_of_the_written_elements(name):
    p, c0 = R.case(name)
    want, bound, written = R.apply(c0, p)
    seen = []
    for mname, wrong in R.mutants(p):
        bad = wrong(c0)
        outside = ~(np.abs(bad[written] - want[written]) <= bound[written])
        frac = float(outside.mean())
        seen.append(mname)
        print("[sgemm-ref] %s: mutant %s outside the bound in %.1f %% of %d written elements" % (name, mname, 100 * frac, outside.size))
        assert frac >= 0.5, (name, mname, frac)
    assert "drop_k" in seen
    assert ("slice_overlap" in seen) == (R.part_elems(p) > 0)
    assert ("beta_dropped" in seen) == (p["beta"] != 0)
    assert ("bias_prev_batch" in seen) == (p["bias"] is not None and p["batch"] > 1)
    assert ("ldc_is_N" in seen) == (p["ldc"] > p["N"] and p["M"] > 1)


def test_every_mutant_is_applied_somewhere():
    names = set()
    for name in R.CASES:
        names |= {m for m, _ in R.mutants(R.case(name)[0])}
    assert names == {"drop_k", "drop_last_pair", "slice_overlap", "bias_prev_batch", "row_shift", "beta_dropped", "ldc_is_N"}


def test_effective_split_literals():
    assert R.effective_split(16, 8) == (16, 1)
    assert R.effective_split(17, 8) == (16, 2)
    assert R.effective_split(33, 2) == (32, 2)
    assert R.effective_split(130, 2) == (80, 2)
    assert R.effective_split(300, 8) == (48, 7)
    assert R.effective_split(600, 8) == (80, 8)
    assert R.effective_split(1000, 8) == (128, 8)
    assert R.effective_split(77, 1) == (77, 1) and R.effective_split(77, 0) == (77, 1)
    for K, ks in R.SPLIT_K:
        kchunk, slices = R.effective_split(K, ks)
        assert kchunk % 16 == 0 and (slices - 1) * kchunk < K <= slices * kchunk and slices <= ks


def test_part_elems():
    p, _ = R.case("split/dW_K300_ks8_batch3")
    assert R.part_elems(p) == 7 * 3 * 33 * 65
    p, _ = R.case("split/dW_K16_ks8_batch3")
    assert R.part_elems(p) == 0
    p, _ = R.case("edge/M33_N65_K65")
    assert R.part_elems(p) == 0


def test_written_mask():
    M, N = 6, 4
    p, c0 = R.make(M, N, 3, ldc_pad=5)
    _, bound, w = R.apply(c0, p)
    body = w[R.GUARD:len(c0) - R.GUARD]
    assert not w[:R.GUARD].any() and not w[-R.GUARD:].any() and len(body) == (M - 1) * (N + 5) + N
    rows = np.concatenate([body, np.zeros(5, bool)]).reshape(M, N + 5)
    assert rows[:, :N].all() and not rows[:, N:].any() and (~rows).sum() == 5 * M
    assert (bound[~w] == 0).all() and (bound[w] > 0).all()

    p, c0 = R.make(M, N, 3, batch=3, c_gap=7)
    assert p["sC"] == M * N + 7
    _, _, w = R.apply(c0, p)
    body = np.concatenate([w[R.GUARD:len(c0) - R.GUARD], np.zeros(7, bool)]).reshape(3, M * N + 7)
    assert body[:, :M * N].all() and not body[:, M * N:].any()

    p, c0 = R.make_score(C=5, D=8, Bn=1)
    assert (p["ldc"], p["N"], p["M"]) == (1, 1, 5)
    _, _, w = R.apply(c0, p)
    assert w[R.GUARD:R.GUARD + 5].all() and w.sum() == 5
    p, c0 = R.make_score(C=5, D=8, Bn=4)
    _, _, w = R.apply(c0, p)
    assert w[R.GUARD:R.GUARD + 20].all() and w.sum() == 20 and len(c0) == 20 + 2 * R.GUARD


def _view(buf, off, s, rs, cs, Z, Rn, K):
    """The operand as numpy sees a strided view of the flat buffer (float64 copy)."""
    it = buf.itemsize
    return np.lib.stride_tricks.as_strided(buf[off:], shape=(Z, Rn, K), strides=(s * it, rs * it, cs * it)).astype(f64)


@pytest.mark.parametrize("name", ["stride/Ak_Bk_M65_N33_K67", "stride/Ak_Br_M65_N33_K67", "stride/Ar_Bk_M65_N33_K67", "stride/Ar_Br_M65_N33_K67",
                                  "stride/A_general_cs2_rs2K+3", "stride/A_padded_row_rsK+5", "layout/stage1_teacher_side_score_ldc1_N1",
                                  "layout/shared_A_sA0_batch3", "split/kfast_K300_ks8_batch3_bias_alpha_beta_ldc_gap"])
def test_reference_equals_einsum_on_strided_views(name):
    p, c0 = R.case(name)
    Z, M, N, K = p["batch"], p["M"], p["N"], p["K"]
    A = _view(p["A"], p["a_off"], p["sA"], p["a_rs"], p["a_cs"], Z, M, K)
    B = _view(p["B"], p["b_off"], p["sB"], p["b_rs"], p["b_cs"], Z, N, K)
    C = np.lib.stride_tricks.as_strided(c0[p["c_off"]:], shape=(Z, M, N), strides=(4 * p["sC"], 4 * p["ldc"], 4)).astype(f64)
    v = p["alpha"] * np.einsum("zmk,znk->zmn", A, B)
    if p["bias"] is not None:
        v += np.stack([p["bias"][p["bias_off"] + z * p["sBias"]:][:N] for z in range(Z)]).astype(f64)[:, None, :]
    if p["beta"] != 0:
        v += p["beta"] * C
    want, _, written = R.apply(c0, p)
    got = np.lib.stride_tricks.as_strided(want[p["c_off"]:], shape=(Z, M, N), strides=(8 * p["sC"], 8 * p["ldc"], 8))
    np.testing.assert_allclose(got, v, rtol=1e-13, atol=1e-13)
    assert written.sum() == Z * M * N and np.array_equal(want[~written], c0[~written].astype(f64))


def test_cases_keep_rows_and_members_distinct():
    """A row or batch mix-up has to change values: no two rows of A, no two members' biases are equal (shared operands aside)."""
    for name in R.CASES:
        p, _ = R.case(name)
        A, B, bias, _ = R.operands(p)
        rows = A.reshape(-1, p["K"]) if p["sA"] else A[0]
        assert len(np.unique(rows, axis=0)) == len(rows), name
        if p["bias"] is not None and p["batch"] > 1:
            assert len(np.unique(bias, axis=0)) == p["batch"], name


def test_groups_name_cases():
    for g in R.GROUPS.values():
        assert 1 <= len(g) <= 8 and all(n in R.TABLE for n in g)
    assert len(R.GROUPS["one"]) == 1 and len(R.GROUPS["eight"]) == 8
    split = [R.part_elems(R.case(n)[0]) > 0 for n in R.GROUPS["alternate"]]
    assert split == [False, True, False, True, True, False]
    assert [R.part_elems(R.case(n)[0]) for n in R.GROUPS["fallback"]] == [0, 0, 0]
    assert [R.case(n)[0]["ksplit"] for n in R.GROUPS["fallback"]] == [1, 8, 1]
