"""CPU: the shapes and schedules of tests/stage1_history_ref.py reach what they claim (integer arithmetic, the records themselves and
one run of the numpy oracle).  A schedule that stops covering a hazard fails here instead of passing quietly on the GPU
(tests/test_stage1_history_gpu.py)."""
import numpy as np

import stage1_history_ref as SR
import widths_ref as W

A_, B_, C_ = SR.SCHEDULE_A, SR.SCHEDULE_B, SR.SCHEDULE_C


def _pairs(schedule):
    return list(zip(schedule, schedule[1:]))


def _has_pair(schedule, a, b):
    """Two consecutive records with a(first) and b(second)."""
    return any(a(x) and b(y) for x, y in _pairs(schedule))


def test_shapes_give_the_rows_the_schedules_are_here_for():
    assert SR.rows(SR.B_FULL) == (408, 432, 840) and [r % 64 for r in SR.rows(SR.B_FULL)] == [24, 48, 8]
    assert SR.rows(SR.B_SHORT) == (272, 288, 560) and [r % 64 for r in SR.rows(SR.B_SHORT)] == [16, 32, 48]
    assert SR.rows(SR.B_FULL)[0] % 32 == 24 and SR.rows(SR.B_SHORT)[0] % 32 == 16        # where the body part of a joint pass starts
    assert SR.LB > SR.AP_LONG and SR.LB % SR.AP_LONG == 8 and -(-SR.LB // 32) * 32 == 96  # chunked pooling, an 8-token last chunk ; Lr
    assert SR.LT <= 32                                                                    # the short attention kernels
    assert SR.H % 256 == 0 and SR.I % 256 == 0 and SR.H == 64 * SR.A                      # _joint_ok's tiling rule
    assert SR.TR == (0, 1) and SR.NL == 2 and SR.T_ == 2 and (SR.D, SR.Q, SR.VOCAB, SR.MAX_POS) == (64, 72, 2000, 128)
    assert SR.MAX_POS >= SR.LB


def test_tables_and_feeds():
    tt, tb = SR.table("title"), SR.table("body")
    assert tt.shape == (301, 2 * SR.LT) and tb.shape == (301, 2 * SR.LB) and tt.dtype == tb.dtype == np.int32
    assert not tt[0].any() and not tb[0].any() and tt[:, :SR.LT].max() < SR.VOCAB and tb[:, :SR.LB].max() < SR.VOCAB
    lens = tb[:, SR.LB:].sum(1)
    assert (lens > SR.AP_LONG).sum() >= 20 and (lens[1:] < SR.AP_LONG).sum() >= 20       # bodies that reach into the last chunk, and not
    assert SR.teachers("title").shape == SR.teachers("body").shape == (SR.T_, 301, SR.D)
    assert SR.teachers("title").dtype == np.float32 and not np.array_equal(SR.teachers("title"), SR.teachers("body"))
    for n in (SR.B_FULL * SR.C, SR.B_SHORT * SR.C, SR.B_FULL, SR.B_SHORT):                # encode_table ends on a partial pass
        assert 301 % n != 0
    assert sorted(SR.FEEDS) == ["full_a", "full_b", "full_c", "short_a", "short_b"]
    seen = []
    for fid, B in SR.FEEDS.items():
        idx, y = SR.feed(fid)
        assert idx.shape == (B, SR.C) and idx.dtype == np.int32 and 1 <= idx.min() and idx.max() <= SR.N_DOCS
        assert y.shape == (B,) and y.dtype == np.int64 and 0 <= y.min() and y.max() < SR.C
        assert all(not np.array_equal(idx, o[:B]) for o in seen)                          # unlike each other
        seen.append(idx)
    assert len({tuple(SR.feed(f)[1]) for f in SR.FEEDS}) >= 4


def test_token_form_is_the_indexed_feed():
    title, body, y, tt, tb = SR.tokens("short_a")
    idx, y2 = SR.feed("short_a")
    assert title.shape == (SR.B_SHORT, SR.C, 2 * SR.LT) and body.shape == (SR.B_SHORT, 2 * SR.LB) and title.dtype == body.dtype == np.int64
    assert np.array_equal(title[2, 3], SR.table("title")[idx[2, 3]]) and np.array_equal(body[3], SR.table("body")[idx[3, 0]])
    assert len(tt) == len(tb) == SR.T_ and tt[0].shape == (SR.B_SHORT, SR.C, SR.D) and tb[0].shape == (SR.B_SHORT, SR.D)
    assert np.array_equal(tt[1][0, 2], SR.teachers("title")[1, idx[0, 2]]) and np.array_equal(tb[1][1], SR.teachers("body")[1, idx[1, 0]])
    assert y is y2


def test_schedule_a_holds_every_listed_pair():
    j, pp = (lambda r: r["joint"]), (lambda r: not r["joint"])
    hk, nh = (lambda r: r["hook"]), (lambda r: not r["hook"])
    full, short = (lambda r: r["B"] == SR.B_FULL), (lambda r: r["B"] == SR.B_SHORT)
    both = lambda *fs: (lambda r: all(f(r) for f in fs))
    # joint -> joint with hook -> per-pass -> per-pass with hook (the chained, hooked form) -> joint
    assert [(r["joint"], r["hook"]) for r in A_[:5]] == [(True, False), (True, True), (False, False), (False, True), (True, False)]
    assert all(full(r) for r in A_[:5]) and A_[3]["chain_wgrad"] and A_[3]["two_streams"]
    # full -> short joint in tok form (the anchor) -> short per-pass -> short joint with hook -> full in tok form
    i, = [i for i, r in enumerate(A_) if r["anchor"]]
    assert full(A_[i - 1]) and [(r["B"], r["joint"], r["hook"], r["form"]) for r in A_[i:i + 4]] == [
        (SR.B_SHORT, True, False, "tok"), (SR.B_SHORT, False, False, "idx"), (SR.B_SHORT, True, True, "idx"), (SR.B_FULL, True, False, "tok")]
    # encode_table of both tables in front of a per-pass step, and again in front of a joint step
    enc = [r for r in A_ if r["pre"]]
    assert [r["pre"] for r in enc] == [tuple(SR.BOTH)] * 2 and [r["joint"] for r in enc] == [False, True]
    assert set(SR.BOTH) == {("encode_table", "title"), ("encode_table", "body")}
    assert all(any(x["joint"] for x in A_[:A_.index(r)]) for r in enc)                    # joint rows lie in the buffers they run through
    # two_streams off under per-pass, joint_streams on under joint ; never elsewhere
    assert [r["joint"] for r in A_ if not r["two_streams"]] == [False] and [r["joint"] for r in A_ if r["joint_streams"]] == [True]
    # chain_wgrad off after chained steps, and chained again behind it
    k, = [i for i, r in enumerate(A_) if not r["chain_wgrad"]]
    assert pp(A_[k]) and any(pp(r) and r["chain_wgrad"] for r in A_[:k]) and pp(A_[k + 1]) and A_[k + 1]["chain_wgrad"]
    # each direction of every switch between consecutive steps
    assert _has_pair(A_, j, pp) and _has_pair(A_, pp, j) and _has_pair(A_, both(j, nh), both(j, hk)) and _has_pair(A_, both(pp, hk), j)
    assert _has_pair(A_, full, short) and _has_pair(A_, short, full) and _has_pair(A_, both(short, j), both(short, pp))
    assert {r["form"] for r in A_} == set(SR.FORMS)
    # the first step again at the end, for both types
    for dtype in ("bf16", "fp16"):
        recs = SR.steps_for(A_, dtype)
        same = lambda a, b: all(a[k] == b[k] for k in a if k not in ("only", "mult")) and b["mult"] == 1.0
        assert same(recs[0], recs[-1]) and len(recs) == len(A_) - (4 if dtype == "bf16" else 0), dtype
    assert all(r["drop"] is None for r in A_) and not any(a[0] == "step" for r in A_ for a in r["pre"])


def test_schedule_a_scale_steps_replay_a_recorded_key_in_both_forms():
    sc = [r for r in A_ if r["only"] == "fp16"]
    assert [(r["joint"], r["mult"]) for r in sc] == [(False, 0.5), (False, 1.0), (True, 0.5), (True, 1.0)]
    assert all(r["only"] is None and r["mult"] == 1.0 for r in A_ if r not in sc) and {r["only"] for r in A_} == {None, "fp16"}
    ep = SR.epochs(A_)
    for first in (sc[0], sc[2]):
        i = A_.index(first)
        assert A_[i + 1] is sc[sc.index(first) + 1] and ep[i] == ep[i + 1]
        # the key was recorded at scale 1 earlier in the same workspace
        assert any(ep[n] == ep[i] and SR.key_form(A_[n]) == SR.key_form(first) and A_[n]["mult"] == 1.0 for n in range(i)), i
    # the epochs themselves: the batch moves twice, three per-pass steps follow a joint one at the full batch and one at the short
    assert ep[0] == 0 and ep[-1] == len([1 for a, b in _pairs(A_) if a["B"] != b["B"] or (a["joint"] and not b["joint"])])
    assert SR.steps_for(A_, "bf16") == [r for r in A_ if r["only"] is None]


def test_anchor_step_and_its_oracle():
    i, = [i for i, r in enumerate(A_) if r["anchor"]]
    r = A_[i]
    assert i == 5 and r["B"] == SR.B_SHORT and r["form"] == "tok" and r["joint"] and not r["hook"] and r["drop"] is None
    assert all(x["only"] is None for x in A_[:i])                                         # the same steps in front of it in both builds
    out, G = SR.anchor_oracle()
    for k in ("distill_loss", "target_loss", "emb_loss", "total_loss"):
        assert np.isfinite(float(out[k])), k
    assert out["student_score"].shape == (SR.B_SHORT, SR.C) and np.isfinite(out["student_score"]).all()
    assert out["title_vec"].shape == (SR.B_SHORT, SR.C, SR.D) and out["body_vec"].shape == (SR.B_SHORT, SR.D)
    assert any("encoder.layer.0." in k for k in G) and any("encoder.layer.1." in k for k in G) and any("transform_matrix" in k for k in G)
    assert not any("user_encoder" in k or k.startswith("teachers.") for k in G)           # DistillModel's schema
    for k, g in G.items():                                                                # the rules of tests/widths_ref.py
        assert np.isfinite(g).all(), k
        if k.endswith(W.NOOP):
            assert np.abs(g).max() < 1e-6, k
        else:
            assert np.sqrt((g.astype(np.float64) ** 2).sum()) >= W.MIN_NORM, k


def test_schedule_b_toggles_dropout():
    on = [r["drop"] is not None for r in B_]
    assert on == [False, True, True, True, True, False]
    assert [(r["B"], r["joint"]) for r in B_] == [(6, True), (6, True), (4, True), (4, False), (6, True), (6, True)]
    assert [r["pre"] for r in B_ if r["pre"]] == [tuple(SR.BOTH)] and B_[4]["pre"] and on[4]      # eval passes with dropout set
    assert all(r["drop"] in (None, SR.DROP) for r in B_) and min(SR.DROP[:2]) > 0
    assert all(B_[0][k] == B_[-1][k] for k in B_[0])                                      # off again on the first step's feed
    assert all(r["only"] is None and not r["hook"] for r in B_)


def test_schedule_c_moves_the_weights_between_unlike_steps():
    assert [(r["B"], r["joint"], r["hook"]) for r in C_] == [(6, True, False), (4, False, False), (6, True, True), (6, True, False)]
    assert C_[0]["pre"] == () and all(r["pre"] == (("step", SR.LR),) for r in C_[1:])
    assert len({r["feed"] for r in C_}) == 4 and all(r["drop"] is None and r["only"] is None for r in C_)
    # an update of about lr per element is several ulps of the 16-bit copies
    w = SR.weights()[W.BERT + "encoder.layer.1.attention.self.query.weight"]
    assert SR.LR > 4 * 2.0 ** -8 * np.median(np.abs(w))
