"""CPU: what tests/test_variants_gpu.py rests on (tests/variants_ref.py) - the boosted weights leave no oracle gradient below the
noise floor, the key sets agree, the name-derived rate and decay tables are what three contiguous rate ranges can serve, and the
schedules of tests/history_ref.py still reach what they claim."""
import numpy as np
import pytest

import history_ref as HR
import variants_ref as V
import widths_ref as W
from oracle import newsrec_oracle as O

RATES = (2e-2, 1e-2, 5e-3)          # lr, lr_bert, lr_news_head: all different
_ENG = {}


def _cpu_engine(v):
    """An engine on the CPU for its slot table (as tests/test_ema_cpu.py builds one): no kernel runs."""
    if v not in _ENG:
        import engine as E
        _ENG[v] = E.Engine(E.EngineConfig(**V.engine_kwargs(v)), device="cpu", max_batch=1)
    return _ENG[v]


def test_the_variants_are_the_ones_history_ref_leaves_out():
    assert V.VARIANTS["att"] == dict(pooling=HR.oracle_cfg()["pooling"], nrms=HR.oracle_cfg()["nrms_heads"], ulm=HR.oracle_cfg()["user_log_mask"])
    new = [V.VARIANTS[v] for v in V.NEW]
    assert {c["pooling"] for c in new} == {"att", "cls", "mean"} and {c["ulm"] for c in new} == {True, False}
    assert any(c["nrms"] and c["ulm"] for c in new) and any(c["nrms"] and not c["ulm"] for c in new) and any(not c["nrms"] for c in new)
    assert all(c["nrms"] * 16 in (0, HR.D) for c in new)
    for v in V.VARIANTS:
        P = V.weights(v)
        assert all(w.dtype == np.float32 for w in P.values())
        n = [k for k in P if V.boosted(k)]
        # the student's user encoder (pooling fc1 / fc2, NRMS W_Q / W_K / W_V) and the news encoder's dense: no teacher, no bias
        assert len(n) == 3 + 3 * bool(V.VARIANTS[v]["nrms"]) and not any(k.startswith("teachers.") or k.endswith("bias") for k in n)


@pytest.mark.parametrize("v", list(V.VARIANTS))
def test_no_gradient_is_below_the_floor(v):
    """Every oracle gradient key of the anchor feed is in exactly one group: a mathematical no-op (widths_ref.NOOP), pad_doc under
    user_log_mask (exactly zero), or at least 1e-4 of the largest norm.  No key is passed over for being small.  The plan step's
    feed (p64_a) is held to the same condition: the GPU file compares it key by key as well."""
    c = V.VARIANTS[v]
    for fid in (V.anchor_feed(), "p64_a"):
        ref_l, ref_s, G, un = V.oracle(v, fid)
        assert np.isfinite(ref_l).all() and np.isfinite(ref_s).all() and all(np.isfinite(g).all() for g in G.values())
        norms = {k: V.norm(g) for k, g in G.items()}
        top = max(norms.values())
        small, groups = None, dict(noop=0, zero=0)
        for k, g in G.items():
            how = V.exempt(v, k)
            if how == "noop":
                assert np.abs(g).max() < 1e-6, (k, np.abs(g).max())
                groups["noop"] += 1
            elif how == "zero":
                assert np.abs(g).max() == 0.0, k
                groups["zero"] += 1
            else:
                assert norms[k] >= V.FLOOR * top, "%s %s: %s has norm %.2e of %.2e" % (v, fid, k, norms[k], top)
                small = norms[k] if small is None else min(small, norms[k])
        print("\n[variants %s %s] smallest non-exempt norm %.2e, largest %.2e, max |score| %.2f, max |user|_2 %.2f" % (
            v, fid, small, top, np.abs(ref_s).max(), un))
        # key.bias of the trainable layer, fc2.bias of the user pooling (+ the news pooling's under 'att'), W_K.bias under NRMS
        assert groups == dict(noop=2 + (c["pooling"] == "att") + bool(c["nrms"]), zero=int(c["ulm"]))
        assert ref_s.shape == (HR.FEEDS[fid][0], HR.C) and V.score_den(v, ref_s, un) >= 1.0


@pytest.mark.parametrize("v", list(V.VARIANTS))
def test_key_sets(v):
    """state_shapes' keys are the oracle's gradient keys plus the frozen ones, and the engine's schema and trainable set agree."""
    import engine as E
    P, G = V.weights(v), V.oracle(v, V.anchor_feed())[2]
    cfg = E.EngineConfig(**V.engine_kwargs(v))
    frozen = {k for k in P if not E.is_trainable(cfg, k)}
    assert set(P) == set(G) | frozen and not set(G) & frozen
    shapes = E.param_shapes(cfg)
    assert set(shapes) == set(P) and all(tuple(shapes[k]) == P[k].shape == (G[k].shape if k in G else P[k].shape) for k in P)
    eng = _cpu_engine(v)
    assert set(eng.grads) == set(G)
    has = lambda s: any(s in k for k in G)
    assert has("attn.att_fc1.weight") and has(V.UE + "pad_doc")
    assert has(O.PFX + "attn.att_fc1.weight") == (V.VARIANTS[v]["pooling"] == "att")
    assert has("multi_head_self_attn.W_Q.weight") == bool(V.VARIANTS[v]["nrms"])


@pytest.mark.parametrize("v", list(V.VARIANTS))
def test_rate_and_decay_tables_by_name(v):
    """Over the variant's slot table the name-derived rates take at most three values in contiguous runs of parameters (what
    step()'s three ranges can serve), in the order lr_bert, lr_news_head, lr; the decay mask has a bit in every run that holds a
    2-D weight and none outside a slot; the first gradient bucket starts where the names leave `.bert_model.`."""
    eng = _cpu_engine(v)
    tr = V.trainable(eng.slot)
    n = eng.n_train
    seq = [V.rate_of(k, RATES) for k, _, _, _ in tr]
    runs = [r for i, r in enumerate(seq) if i == 0 or seq[i - 1] != r]
    assert runs == [RATES[1], RATES[2], RATES[0]], runs
    lr, mask, inside = V.rate_table(eng.slot, n, RATES), V.decay_table(eng.slot, n), V.slot_mask(eng.slot, n)
    assert lr.shape == mask.shape == inside.shape == (n,) and set(np.unique(lr)) == set(RATES)
    assert (lr[~inside] == RATES[0]).all() and not mask[~inside].any() and (~inside).any()
    for rate in RATES:
        keys = [(k, shp) for k, _, _, shp in tr if V.rate_of(k, RATES) == rate]
        assert any(len(shp) == 2 and k.endswith(".weight") for k, shp in keys)
        assert mask[inside & (lr == rate)].any() and not mask[inside & (lr == rate)].all()      # 2-D weights decay, biases do not
    head = V.head_elements(eng.slot, n)
    assert np.array_equal(head, inside & (lr == RATES[2]))
    want_head = {O.PFX + "dense.weight", O.PFX + "dense.bias"} | (
        {O.PFX + "attn.att_fc%d.%s" % (i, w) for i in (1, 2) for w in ("weight", "bias")} if V.VARIANTS[v]["pooling"] == "att" else set())
    assert {k for k, _, _, _ in tr if V.rate_of(k, RATES) == RATES[2]} == want_head
    # NRMS's projections decay, their biases do not
    for k, o, cnt, shp in tr:
        if "multi_head_self_attn" in k:
            assert mask[o:o + cnt].all() == k.endswith(".weight") and mask[o:o + cnt].any() == k.endswith(".weight"), k
    first_head = min(o for k, o, _, _ in tr if ".bert_model." not in k)
    br = eng.bucket_ranges()
    assert br[0] == (first_head, n) and len(br) == 1 + 2 * len(HR.TR)
    assert max(o + cnt for k, o, cnt, _ in tr if ".bert_model." in k) <= first_head


def test_why_cls_nrms_takes_a_smaller_factor():
    """At factor 4 the oracle's own W_K.bias gradient of cls_nrms is above the no-op bound: sums of exp() near the 1e-8 of the
    denominator, attention rows that no longer sum to one.  At the factor in use it is rounding noise (the test above)."""
    import hashinit
    from schema import state_shapes
    v = "cls_nrms"
    assert V.BOOST[v] == 2.0 and all(V.BOOST[x] == 4.0 for x in V.VARIANTS if x != v)
    P = hashinit.init_state_dict(91, state_shapes(HR.dims(), HR.NL, HR.D, HR.T_, "cls", 4))
    P = {k: (w * np.float32(4.0) if V.boosted(k) else w) for k, w in P.items()}
    out = O.model_fwd(P, V.oracle_cfg(v), *HR.tokens(V.anchor_feed()))
    G = O.model_bwd(P, V.oracle_cfg(v), out)
    assert np.abs(G[V.UE + "multi_head_self_attn.W_K.bias"]).max() > 10 * W.NOOP_ABS


@pytest.mark.parametrize("v", V.EMBED)
def test_port_with_the_pooling_swapped_agrees_with_the_oracle(v):
    """variants_ref.port_grads (torch autograd through oracle/torch_port.py with x[:, 0] / x.mean(1) as the pooling) against the
    numpy oracle on the anchor feed, within the bounds of tests/test_widths_ref_cpu.py: total loss and scores rtol 2e-4 atol 2e-5,
    gradient norms rtol 1e-3, worst relative L2 of a gradient below 1e-3.  The embedding block's five gradients are the port's
    alone (the oracle stops above them); the word table's has a zero row 0 and zero rows for every word the feed does not name."""
    from embed_train_ref import EMB_KEYS, WORD
    assert not V.VARIANTS[v]["nrms"] and V.VARIANTS[v]["pooling"] != "att"
    fid = V.anchor_feed()
    total, score, Gp = V.port_grads(v, fid)
    ref_l, ref_s, G, _ = V.oracle(v, fid)
    np.testing.assert_allclose(ref_l[0] + V.oracle_cfg(v)["coef"] * ref_l[1] + ref_l[2], total, rtol=2e-4, atol=2e-5)
    np.testing.assert_allclose(ref_s, score, rtol=2e-4, atol=2e-5)
    unused = {k for k in G if V.exempt(v, k) == "zero"}
    assert set(G) - unused == set(Gp) - set(EMB_KEYS) and set(EMB_KEYS) <= set(Gp)
    worst, wk = 0.0, ""
    for k in set(G) - unused:
        if V.exempt(v, k) == "noop":
            assert np.abs(Gp[k]).max() < 1e-6, k
            continue
        np.testing.assert_allclose(V.norm(G[k]), V.norm(Gp[k]), rtol=1e-3, err_msg=k)
        err = W.rel_l2(G[k], Gp[k])
        worst, wk = max((worst, wk), (err, k))
    print("\n[variants %s] oracle vs port with the pooling swapped: worst gradient relative L2 %.2e (%s)" % (v, worst, wk[-48:]))
    assert worst < 1e-3
    named = np.setdiff1d(np.unique(HR.tokens(fid)[0][..., :HR.L].reshape(-1).tolist() + HR.tokens(fid)[2][..., :HR.L].reshape(-1).tolist()), [0])
    rows = np.nonzero(np.abs(Gp[WORD]).max(1))[0]
    assert np.array_equal(rows, named) and 0 not in rows
    assert all(V.norm(Gp[k]) > 1e-4 * max(V.norm(g) for g in Gp.values()) for k in EMB_KEYS)


def test_the_schedules_still_reach_what_they_claim():
    """The feeds, plans, token forms and schedules are history_ref's, unchanged; its own checks are called, not copied.  None of
    them depends on the pooling or the user encoder."""
    import test_history_ref_cpu as TH
    TH.test_feeds_give_the_plans_they_are_named_for()
    TH.test_plain_batches_have_a_tail_inside_their_last_tile()
    TH.test_token_form_is_the_indexed_feed()
    TH.test_schedule_a_reaches_every_hazard()
    TH.test_schedule_a_window_and_scale_steps()
    i, = [i for i, r in enumerate(HR.SCHEDULE_A) if r["anchor"]]
    assert i == 7 and V.anchor_feed() == "short_a" and HR.FEEDS["short_a"][0] == HR.B_SHORT
    assert HR.plan("p64_a").n_enc == 64 and HR.FEEDS["p64_a"][0] == HR.B_FULL


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_comparison_flags_exactly_the_perturbed_key(dtype):
    """variants_ref.compare_grads on the oracle's own gradients with one tensor off by twice / half the tolerance; a perturbed
    no-op key and a non-zero unused pad_doc are flagged."""
    v = "att_nrms_ulm"
    G = V.oracle(v, V.anchor_feed())[2]
    gtol = W.TOLS[dtype][2]
    rs = np.random.RandomState(3)
    for k in (V.UE + "multi_head_self_attn.W_V.weight", V.UE + "multi_head_self_attn.W_Q.bias", O.PFX + "dense.bias"):
        for factor, want in ((2.0, [k]), (0.5, [])):
            d = rs.randn(*G[k].shape)
            d *= factor * gtol * V.norm(G[k]) / V.norm(d)
            got = dict(G)
            got[k] = G[k].astype(np.float64) + d
            assert V.compare_grads(v, list(G), lambda n: got[n], G, gtol)[2] == want, (k, factor)
    for k, d in ((V.UE + "multi_head_self_attn.W_K.bias", 2 * W.NOOP_ABS), (V.UE + "pad_doc", 1e-30)):
        got = dict(G)
        got[k] = G[k] + np.float32(d)
        assert V.compare_grads(v, list(G), lambda n: got[n], G, gtol)[2] == [k]
