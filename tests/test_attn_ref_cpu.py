"""tests/attn_ref.py (the float64 reference, bounds and rounding model of tests/test_attn_kernels_gpu.py) without a GPU:

  * the reference's inner matrices against dropout_ref.attn_fwd / attn_bwd (tied to the oracle's attention by
    tests/test_dropout_ref_cpu.py) to float64 rounding, and against the oracle's own rel-pos table;
  * the case table holds what it is meant to hold (every L and pair count, the dominant keys dominant, the sharp case in fp16's
    subnormal range, the rising / falling masks rescaling at every tile or never);
  * the float32 rounding model passes every bound on every case in both 16-bit kinds (the bounds are satisfiable), and over the
    whole table its worst err / bound is >= 0.1 for every output (no bound is slack by more than 10 x);
  * every seeded defect of the model fails at least one of attn_ref.failures()' checks - the checks the GPU file applies to the
    kernels - on the case designed for it, and the clean model fails none."""
import functools

import numpy as np
import pytest

import attn_ref as AR
import dropout_ref as DR
import rows_ref as RR


@functools.lru_cache(maxsize=None)
def _case(c, kind):
    inp = AR.inputs(c, kind)
    r = AR.reference(inp)
    return inp, r, AR.bounds(r, kind, c.form), AR.emulate(kind, c.form, inp)


def test_reference_against_dropout_ref():
    c = AR.Case("long", 2, 33, 2, "pad30")
    inp, r, _, _ = _case(c, "f16")
    N, L, A = inp["dims"]
    f = DR.attn_fwd(inp["qkv"], r["madd"], r["rel"], N, L, A)
    dqkv, ds = DR.attn_bwd(f, inp["dctx"])
    close = lambda a, b, what: np.testing.assert_allclose(a, b, rtol=1e-12, atol=1e-12 * np.abs(b).max(), err_msg=what)
    e = np.exp(r["S"] - r["S"].max(-1, keepdims=True))
    close(e / e.sum(-1, keepdims=True), f["p"], "softmax(S) = P")
    close(np.log(e.sum(-1)) + r["S"].max(-1), f["lse"], "lse")
    close(AR.rows(r["ctx"]), f["ctx"], "ctx")
    close(AR.rows(r["P"] @ r["v"]), f["ctx"], "P V")
    close(r["P"] * (r["dP"] - r["delta"][..., None]), ds, "dS = P (dP - delta)")
    close((r["dO"] * r["ctx"]).sum(-1), r["delta"], "delta = sum_d dO O")
    close(np.concatenate([AR.rows(r[n]) for n in ("dq", "dk", "dv")], 1), dqkv, "dqkv")
    close(r["colsum"], dqkv.reshape(N, L, -1).sum(1), "column sums")
    assert (inp["mask_add"][:, L:] == AR.NEG_INF).all() and (inp["rel"][:, L:] == 0).all() and (inp["rel"][:, :, L:] == 0).all()
    assert np.array_equal(RR.r16(inp["qkv"], "f16"), inp["qkv"])          # the reference sees what the kernel sees


def test_case_table():
    l32, lng = AR.L32_CASES, AR.LONG_CASES
    assert {c.L for c in l32} == {1, 2, 4, 5, 8, 9, 16, 17, 31, 32}
    assert {c.N * c.A for c in l32} >= {1, 2, 3, 5, 9} and any(c.A == 12 for c in l32)
    for na in ((1, 1), (1, 2), (1, 3), (5, 1), (3, 3)):
        assert len({c.L for c in l32 if (c.N, c.A) == na}) >= 2, na
    assert {c.L for c in lng} >= {1, 24, 32, 33, 64, 97, 128, 129, 160, 200, 256} and any(c.L in (481, 512) for c in lng)
    assert {c.A for c in lng} == {1, 2, 3, 12} and all(c.N <= 2 for c in lng) and AR.Case("long", 1, 33, 12, "plain") in lng
    kinds = lambda cs: {c.inp for c in cs}
    assert kinds(l32) >= {"plain", "pad30", "allpad", "lastdom", "firstdom", "sharp"}
    assert kinds(lng) >= {"plain", "pad30", "allpad", "leftpad", "lastreal", "lastdom", "firstdom", "rising", "falling", "sharp"}
    assert set(AR.DEFECTS.values()) <= set(AR.CASES)
    for c in AR.CASES:
        inp, r, _, _ = _case(c, "f16")
        if c.inp == "lastdom":
            assert c.L % 32 and (r["P"][..., c.L - 1] >= 0.5).all(), c
        if c.inp == "firstdom":
            assert (r["P"][..., 0] >= 0.5).all(), c
        if c.inp == "sharp":
            assert ((r["P"] > 2.0 ** -24) & (r["P"] < 2.0 ** -14)).any(), c
        if c.inp in ("rising", "falling"):
            tile_max = np.stack([r["S"][..., t:t + 32].max(-1) for t in range(0, c.L, 32)], -1)
            d = np.diff(tile_max, axis=-1)
            assert (d > 0).all() if c.inp == "rising" else (d < 0).all(), c
        if c.inp in ("leftpad", "allpad", "lastreal"):
            assert (r["S"][..., :32].max(-1) < -9000).all(), c


@pytest.mark.parametrize("kind", RR.KINDS)
def test_model_within_bounds_and_bounds_not_slack(kind):
    worst = {}
    for c in AR.CASES:
        inp, r, b, emu = _case(c, kind)
        bad, stats = AR.failures(kind, inp, r, b, emu, emu, tag=AR.case_id(c))
        assert not bad, (AR.case_id(c), kind, bad)
        for n, s in stats.items():
            worst[n] = max(worst.get(n, 0.0), s[1])
    print("[attn-ref] %s worst model err / bound over the table: %s" % (kind, ", ".join("%s %.3f" % kv for kv in sorted(worst.items()))))
    for n in AR.OUTS:
        assert 0.1 <= worst[n] <= 1.0, (n, worst[n])


@pytest.mark.parametrize("kind", RR.KINDS)
def test_every_defect_is_caught(kind):
    table = []
    for defect, c in sorted(AR.DEFECTS.items()):
        inp, r, b, emu = _case(c, kind)
        bad, _ = AR.failures(kind, inp, r, b, AR.emulate(kind, c.form, inp, defect=defect), emu, log=lambda s: None)
        table.append("%-13s %-28s %s" % (defect, AR.case_id(c), " ".join(bad) or "SURVIVED"))
    print("[attn-ref] %s mutant -> failing checks\n%s" % (kind, "\n".join(table)))
    assert not [t for t in table if t.endswith("SURVIVED")], "\n".join(table)
