"""CPU: the schedules of tests/history_ref.py reach what they claim (build_plan and integer arithmetic only).  A schedule that
stops covering a hazard fails here instead of passing quietly on the GPU (tests/test_step_history_gpu.py)."""
import numpy as np

import history_ref as HR
import widths_ref as W

A_, B_, C_ = HR.SCHEDULE_A, HR.SCHEDULE_B, HR.SCHEDULE_C
N_FULL, N_SHORT = HR.B_FULL * (HR.U + HR.C), HR.B_SHORT * (HR.U + HR.C)


def _pairs(schedule):
    return list(zip(schedule, schedule[1:]))


def test_feeds_give_the_plans_they_are_named_for():
    for fid, (B, target) in HR.FEEDS.items():
        h, m, c, y = HR.feed(fid)
        assert h.shape == (B, HR.U) and c.shape == (B, HR.C) and m.shape == (B, HR.U) and y.shape == (B,)
        assert h.dtype == c.dtype == np.int32 and 0 <= min(h.min(), c.min()) and max(h.max(), c.max()) <= HR.N_NEWS
        assert c.min() >= 1 and 0 <= y.min() and y.max() < HR.C
        assert (m.sum(1) == 0).any() and (m.sum(1) > 0).any()              # a fully masked history row, and live ones
        assert (h == 0).sum() >= 2 and not m[h == 0].any()                # padding slots, all masked
        p = HR.plan(fid)
        distinct = np.unique(np.concatenate([h.reshape(-1), c.reshape(-1)])).size
        if target is None:
            assert p is None and (distinct > 128 if B == HR.B_FULL else distinct > 64), fid
        elif target == "q16":
            q = HR.plan(fid, quantum=16)
            assert q is not None and q.n_enc % 16 == 0 and (q.n_enc * HR.L) % 64 != 0, fid       # what the engine must refuse
            assert p is not None and (p.n_enc * HR.L) % 64 == 0
        else:
            assert p is not None and p.n_enc == target and p.n_slots == B * (HR.U + HR.C), fid
            assert (65 <= distinct <= 128) if target == 128 else distinct <= 64
            assert (p.n_enc * HR.L) % 64 == 0 and p.uniq[p.n_unique:].sum() == 0       # no tail behind a plan's rows ; padded with news 0
    assert HR.news().shape == (HR.N_NEWS + 1, 2 * HR.L) and not HR.news()[0].any()
    assert (HR.N_NEWS + 1) % N_FULL != 0 and (HR.N_NEWS + 1) % N_SHORT != 0
    assert HR.teachers().shape == (HR.T_, HR.N_NEWS + 1, HR.D)


def test_plain_batches_have_a_tail_inside_their_last_tile():
    assert HR.rows(HR.B_FULL) == 2550 and HR.rows(HR.B_FULL) % 64 == 54
    assert HR.rows(HR.B_SHORT) == 1700 and HR.rows(HR.B_SHORT) % 64 == 36


def test_token_form_is_the_indexed_feed():
    hist, m, cand, y, th, tc = HR.tokens("short_a")
    h, m2, c, y2 = HR.feed("short_a")
    assert hist.shape == (HR.B_SHORT, HR.U, 2 * HR.L) and cand.shape == (HR.B_SHORT, HR.C, 2 * HR.L) and hist.dtype == np.int64
    assert np.array_equal(hist[2, 5], HR.news()[h[2, 5]]) and np.array_equal(cand[3, 1], HR.news()[c[3, 1]])
    assert len(th) == len(tc) == HR.T_ and np.array_equal(th[1][0, 7], HR.teachers()[1, h[0, 7]]) and th[0].shape == (HR.B_SHORT, HR.U, HR.D)
    assert m is m2 and y is y2


def test_schedule_a_reaches_every_hazard():
    ne = [HR.n_enc(r) for r in A_]
    assert {64, 128, N_FULL, N_SHORT} == set(ne)
    assert any(r["B"] == HR.B_FULL and not r["plan"] and HR.plan(r["feed"]) is None for r in A_)
    assert all(HR.plan(r["feed"]) is None for r in A_ if not r["plan"])        # a plain step is what the loader would feed
    # a plan that shrinks, between consecutive steps of one workspace
    assert any(a["B"] == b["B"] and a["plan"] and b["plan"] and (HR.n_enc(a), HR.n_enc(b)) == (128, 64) for a, b in _pairs(A_))
    # a plain step directly behind a plan, and a plan directly behind a plain step
    assert any(a["plan"] and not b["plan"] and a["B"] == b["B"] for a, b in _pairs(A_))
    assert any(b["plan"] and not a["plan"] and a["B"] == b["B"] for a, b in _pairs(A_))
    # two different plans under one key
    for n in (64, 128):
        us = [HR.plan(r["feed"]).uniq for r in A_ if r["plan"] and r["B"] == HR.B_FULL and HR.n_enc(r) == n]
        assert len(us) >= 2 and any(not np.array_equal(us[0], u) for u in us[1:]), n
    # the short batch between two full ones, with more than one step at it
    Bs = [r["B"] for r in A_]
    first, last = Bs.index(HR.B_SHORT), len(Bs) - 1 - Bs[::-1].index(HR.B_SHORT)
    assert 0 < first < last < len(Bs) - 1 and set(Bs[first:last + 1]) == {HR.B_SHORT}
    assert set(Bs[:first]) == set(Bs[last + 1:]) == {HR.B_FULL}
    # every reduction-table key form at least twice, not in consecutive steps
    forms = {}
    for i, r in enumerate(A_):
        forms.setdefault(HR.key_form(r), []).append(i)
    assert set(forms) == {(64, True), (128, True), (N_SHORT, True), (N_FULL, True), (N_FULL, False)}
    for f, at in forms.items():
        assert len(at) >= 2 and at[-1] - at[0] >= 2, (f, at)
    # ... the per-bucket tables (hook on) replayed inside ONE workspace, with unlike steps between
    hooked = [i for i, r in enumerate(A_) if not HR.key_form(r)[1] and i > last]
    assert len(hooked) >= 2 and hooked[-1] - hooked[0] >= 2
    # both feed forms ; the forward-only paths and the cache in front of a step
    assert {r["form"] for r in A_} == {"idx", "tok"} and any(r["form"] == "tok" and r["B"] == HR.B_FULL for r in A_)
    acts = [a[0] for r in A_ for a in r["pre"]]
    assert acts == ["encode_news", "user_vectors", "build_frozen_cache"]
    i_c, = [i for i, r in enumerate(A_) if ("build_frozen_cache",) in r["pre"]]
    assert A_[i_c]["plan"] and not A_[i_c + 1]["plan"] and A_[i_c]["form"] == A_[i_c + 1]["form"] == "idx"     # both go through the cache
    assert all(r["drop"] is None for r in A_)


def test_schedule_a_window_and_scale_steps():
    win = [r for r in A_ if r["micro"]]
    assert [r["micro"] for r in win] == [(0, 2), (1, 2)] and [HR.n_enc(r) for r in win] == [128, 64]
    assert A_.index(win[1]) == A_.index(win[0]) + 1
    sc = [r for r in A_ if r["only"] == "fp16"]
    assert [r["mult"] for r in sc] == [0.5, 1.0] and len({HR.key_form(r) for r in sc}) == 1 and A_[-2:] == sc
    assert all(r["mult"] == 1.0 and r["only"] is None for r in A_[:-2])
    # the key of the scale steps was recorded at scale 1 earlier in the same workspace
    i0 = A_.index(sc[0])
    since = max(i for i in range(i0) if A_[i]["B"] != sc[0]["B"])
    assert any(HR.key_form(r) == HR.key_form(sc[0]) for r in A_[since + 1:i0])
    for dtype, n in (("bf16", len(A_) - 2), ("fp16", len(A_))):
        w = HR.windows(A_, dtype)
        assert sum(len(x) for x in w) == n and sorted(len(x) for x in w)[-2:] == [1, 2]


def test_anchor_is_the_eighth_step_and_no_gradient_is_passed_over():
    i, = [i for i, r in enumerate(A_) if r["anchor"]]
    r = A_[i]
    assert i == 7 and r["B"] == HR.B_SHORT and r["form"] == "tok" and not r["plan"] and not r["hook"] and r["micro"] is None
    assert all(x["micro"] is None and x["only"] is None for x in A_[:i])      # seven whole steps in front of it, in both builds
    ref_l, ref_s, G = HR.anchor_oracle()
    assert np.isfinite(ref_l).all() and ref_s.shape == (HR.B_SHORT, HR.C)
    import engine as E
    assert set(G) == {k for k in HR.weights() if E.is_trainable(E.EngineConfig(**HR.engine_kwargs()), k)}
    for k, g in G.items():                                                     # the rules of tests/widths_ref.py
        if k.endswith(W.NOOP):
            assert np.abs(g).max() < 1e-6, k
        else:
            assert np.sqrt((g.astype(np.float64) ** 2).sum()) >= W.MIN_NORM, k


def test_schedule_b_toggles_dropout():
    on = [r["drop"] is not None for r in B_]
    assert on == [False, True, True, True, True, False]
    assert [r["B"] for r in B_][1:4] == [HR.B_FULL, HR.B_SHORT, HR.B_FULL]      # on across a new workspace and back
    assert [a for r in B_ for a in r["pre"]] == [("encode_news_eval",)] and B_[3]["pre"] and on[2] and on[3]
    assert all(r["drop"] in (None, HR.DROP) for r in B_) and min(HR.DROP[:2]) > 0


def test_schedule_c_moves_the_weights_between_unlike_steps():
    assert [(r["B"], r["plan"], HR.n_enc(r)) for r in C_] == [(6, True, 128), (4, False, N_SHORT), (6, False, N_FULL), (6, True, 64)]
    assert C_[0]["pre"] == (("build_frozen_cache",),) and all(r["pre"] == (("step", HR.LR),) for r in C_[1:])
    # an update of about lr per element is several ulps of the 16-bit copies (weights of the initialisation: |w| < 0.25)
    w = HR.weights()[HR.BERT + "encoder.layer.1.attention.self.query.weight"]
    assert HR.LR > 4 * 2.0 ** -8 * np.median(np.abs(w))
    # consecutive steps name different words: each step leaves rows of the word table that the next one does not name
    for a, b in _pairs(C_):
        assert np.setdiff1d(HR.named_tokens(a), HR.named_tokens(b)).size > 50
