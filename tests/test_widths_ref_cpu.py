"""CPU: the two references at the encoder widths of tests/widths_ref.py (tests/test_encoder_widths_gpu.py holds the engine to them),
and the comparison helper both files use.

The numpy oracle and the torch port have each been pinned to the reference's goldens at hidden 768 only (tests/test_oracle_golden.py,
rtol 2e-4 / atol 2e-5 on losses and scores, gradient norms rtol 1e-3, gradient elements rtol 2e-3 with an absolute floor of
2e-3 x the tensor's largest element); here they are held to each other within those bounds at 256, 512 and 1024."""
import numpy as np
import pytest

import widths_ref as W
from embed_train_ref import EMB_KEYS, port_grads

RTOL, ATOL = 2e-4, 2e-5      # tests/test_oracle_golden.py


def test_table_covers_every_accepted_width_and_both_kinds_of_inter():
    cs = W.WIDTH_CASES.values()
    assert {(c["H"], c["A"]) for c in cs} == {(256, 4), (512, 8), (768, 12), (1024, 16)}
    for H in (256, 512, 1024):
        kinds = {c["I"] % 256 == 0 for c in cs if c["H"] == H}
        assert kinds == {True, False}, H                                          # a multiple of 256, and 128 x odd
    assert {c["pooling"] for c in cs} == {"att", "cls", "mean"}
    assert any(c["L"] <= 32 for c in cs) and any(32 < c["L"] <= 64 for c in cs) and any(c["L"] > 64 for c in cs)
    assert any(min(c["tr"]) > 0 for c in cs) and any(tuple(c["tr"]) == tuple(range(c["nl"])) for c in cs)
    assert any(W.rows(c) <= 128 for c in cs) and any(W.rows(c) > 128 for c in cs)
    assert any(c["nrms"] and c["nrms"] * 16 == c["D"] for c in cs)
    assert {c["ulm"] for c in cs} == {True, False} and {1, 3} <= {c["T"] for c in cs}
    assert any("pp" in c["routes"].values() and c["H"] == 256 for c in cs)
    for name, c in W.WIDTH_CASES.items():
        assert set(c["routes"]) == {n for n, _, _, _ in W.nt_launches(name)}, name
        assert c["H"] == 64 * c["A"] and c["I"] % 128 == 0 and c["L"] <= W.MAX_POS


def test_engine_config_takes_every_case():
    import engine as E
    for name in W.WIDTH_CASES:
        P, cfg, kw, inp = W.case(name)
        ec = E.EngineConfig(**kw)
        shapes = E.param_shapes(ec)
        assert set(shapes) == set(P), name
        for k, v in P.items():
            assert tuple(shapes[k]) == v.shape, (name, k)


@pytest.mark.parametrize("name", list(W.WIDTH_CASES))
def test_no_gradient_is_silently_passed_over(name):
    """The condition the GPU test rests on: apart from the keys W.exempt() names - the mathematical no-ops, and pad_doc where
    user_log_mask leaves it unused (exactly zero) - every gradient of the oracle has a norm of at least 1e-7, so a relative
    bound on all the others passes over nothing; and the exempt ones are what their check assumes."""
    _, _, G = W.oracle(name)
    top = max(np.sqrt((g.astype(np.float64) ** 2).sum()) for g in G.values())
    assert top > 1e-2
    n_exempt = 0
    for k, g in G.items():
        rn = np.sqrt((g.astype(np.float64) ** 2).sum())
        how = W.exempt(name, k)
        if how is None:
            assert rn >= W.MIN_NORM, "%s: norm %.2e" % (k, rn)
        elif how == "zero":
            assert np.abs(g).max() == 0.0, k
            n_exempt += 1
        else:
            assert k.endswith(W.NOOP) and np.abs(g).max() < 1e-6, "%s: %.2e" % (k, np.abs(g).max())
            n_exempt += 1
    c = W.WIDTH_CASES[name]
    # key.bias per trainable layer, fc2.bias of the user pooling (+ the news pooling's under 'att'), W_K.bias under NRMS, pad_doc
    assert n_exempt == len(c["tr"]) + 1 + (c["pooling"] == "att") + bool(c["nrms"]) + c["ulm"]
    worst, wk, bad = W.compare_grads(name, list(G), lambda k: G[k], G, 1e-12)
    assert bad == [] and worst == 0.0


@pytest.mark.parametrize("name", W.PORT_CASES)
def test_oracle_agrees_with_the_torch_port(name):
    """NAML / attention-pooling cases only: oracle/torch_port.py has neither the NRMS user encoder nor cls / mean pooling, so
    h512_i1152_l40 and h256_i640_l33 rest on the oracle alone (as the goldens' variants 3 and 4 do at 768)."""
    P, cfg, _, inp = W.case(name)
    ref_l, ref_s, G = W.oracle(name)
    total, score, Gp = port_grads(P, cfg, *inp)
    np.testing.assert_allclose(ref_l[0] + cfg["coef"] * ref_l[1] + ref_l[2], total, rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(ref_s, score, rtol=RTOL, atol=ATOL)
    unused = {k for k in G if W.exempt(name, k) == "zero"}                    # autograd leaves .grad None: the oracle says 0
    assert set(G) - unused == set(Gp) - unused - set(EMB_KEYS)             # port_grads adds the embedding block's
    # the no-op keys' gradients are pure fp32 rounding noise: they measure the noise floor of their block, as in
    # tests/test_oracle_golden.py (a bias gradient that is a sum of cancelling terms sits only a decade or two above it)
    block = lambda n: "user" if n.startswith("student.user_encoder.") else "news"
    floor = {"user": 0.0, "news": 0.0}
    for k in G:
        if W.exempt(name, k) == "noop":
            floor[block(k)] = max(floor[block(k)], float(np.abs(Gp[k]).max()), float(np.abs(G[k]).max()))
    worst, wk = 0.0, ""
    for k, g in G.items():
        if k in unused:
            assert np.abs(g).max() == 0.0 and (k not in Gp or np.abs(Gp[k]).max() == 0.0), k
            continue
        if W.exempt(name, k) is not None:
            assert np.abs(g).max() < 1e-6 and np.abs(Gp[k]).max() < 1e-6, k
            continue
        ref, nf = Gp[k], 4.0 * floor[block(k)]
        np.testing.assert_allclose(np.sqrt((g.astype(np.float64) ** 2).sum()), np.sqrt((ref.astype(np.float64) ** 2).sum()), rtol=1e-3,
                                   atol=1e-9 + nf * np.sqrt(g.size), err_msg=k)
        np.testing.assert_allclose(g, ref, rtol=2e-3, atol=2e-3 * float(np.abs(ref).max()) + 1e-10 + nf, err_msg=k)
        err = W.rel_l2(g, ref)
        if err > worst:
            worst, wk = err, k
    print("\n[%s] oracle vs port: worst gradient relative L2 %.2e (%s)" % (name, worst, wk))
    assert worst < 1e-3          # the references' own disagreement stays a twentieth of the tightest bound the engine is held to


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_comparison_flags_exactly_the_perturbed_key(dtype):
    """The helper on the oracle's own gradients with ONE tensor off by twice the gradient tolerance (relative L2): that key and no
    other; at half the tolerance: none.  A perturbed no-op key or a non-zero unused pad_doc is flagged as well."""
    name = "h256_i384_l19"
    _, _, G = W.oracle(name)
    gtol = W.TOLS[dtype][2]
    rs = np.random.RandomState(3)
    for k in (W.BERT + "encoder.layer.1.intermediate.dense.weight", W.BERT + "encoder.layer.1.attention.self.query.bias",
              "student.user_encoder.attn.att_fc1.bias", "transform_matrix.1.weight"):
        for factor, want in ((2.0, [k]), (0.5, [])):
            d = rs.randn(*G[k].shape)
            d *= factor * gtol * np.sqrt((G[k].astype(np.float64) ** 2).sum()) / np.sqrt((d ** 2).sum())
            got = dict(G)
            got[k] = G[k].astype(np.float64) + d
            worst, wk, bad = W.compare_grads(name, list(G), lambda n: got[n], G, gtol)
            assert bad == want, (k, factor, bad)
            assert wk == k and abs(worst - factor * gtol) < 1e-6 * gtol
    for k, d in ((W.BERT + "encoder.layer.1.attention.self.key.bias", 2 * W.NOOP_ABS), ("student.user_encoder.pad_doc", 1e-30)):
        got = dict(G)
        got[k] = G[k] + np.float32(d)
        assert W.compare_grads(name, list(G), lambda n: got[n], G, gtol)[2] == [k]
