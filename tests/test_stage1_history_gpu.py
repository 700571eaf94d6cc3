"""GPU: a stage-1 training step does not depend on the steps before it.

One long-lived Stage1Engine is driven through the schedules of tests/stage1_history_ref.py (pinned by
tests/test_stage1_history_ref_cpu.py): the joint and the per-pass form in both orders, a bucket hook on and off, the short batch
and the way back (the body rows move from row 408 to row 272 of the title engine's buffers), all three feed forms, eval passes over
both tables between steps, every stream / chaining switch, a loss scale that moves under a recorded key in both forms, dropout
toggled across a new workspace, weights that move under the 16-bit copies both engines share.

The rule for every step: after forward + backward on the long-lived engine, a FRESH Stage1Engine of that step's batch size gets the
same weights, switches, dropout, BOTH passes' call numbers and the loss-scale multiplier and runs only that step; ran_joint is as the
record says and the losses, the scores, S[:Rt] and the whole flat_g must be torch.equal.  No tolerance: the joint form equals itself
launch for launch, one stream equals two bit for bit (test_stage1_training_on_two_streams_equals_one_stream_bit_for_bit), no
result depends on the tile plan, so any difference is a dependence on history.  One step - the sixth of schedule A, the first at the
short batch - is held to the numpy oracle as well, under the bounds of tests/test_encoder_widths_gpu.py's stage-1 test."""
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import engine as E                                               # noqa: E402
import stage1_history_ref as SR                                  # noqa: E402
import widths_ref as W                                           # noqa: E402
from stage1 import Stage1Engine                                  # noqa: E402

DEV = "cuda:0"
WHAT = ("losses", "score", "S", "flat_g")
# test_stage1_step_with_dropout_against_the_oracle (tests/test_encoder_widths_gpu.py): losses, scores and news vectors relative to
# max(1, |ref|) ; gradients relative L2 ; no-op keys < W.NOOP_ABS
TOL, GTOL = {"bf16": 1.6e-2, "fp16": 1e-3}, {"bf16": 6e-2, "fp16": 1.5e-2}
_DEV = {}                                                        # device copies of the shared inputs: made once, never modified


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _shared():
    if "P" not in _DEV:
        _DEV.update(P={k: _t(v) for k, v in SR.weights().items()}, title=_t(SR.table("title")), body=_t(SR.table("body")),
                    t_title=_t(SR.teachers("title")), t_body=_t(SR.teachers("body")))
    return _DEV


def _feed(fid, form):
    key = (fid, "tok" if form == "tok" else "idx")
    if key not in _DEV:
        if form == "tok":
            title, body, y, tt, tb = SR.tokens(fid)
            _DEV[key] = (_t(title), _t(body), _t(y), [_t(x) for x in tt], [_t(x) for x in tb])
        else:
            idx, y = SR.feed(fid)
            _DEV[key] = (_t(idx), _t(y), _t(idx[:, 0]))
    return _DEV[key]


def _engine(dtype, B):
    return Stage1Engine(device=DEV, batch=B, dtype=dtype, **SR.engine_kwargs())


def _set(eng, rec):
    eng.joint, eng.two_streams, eng.joint_streams, eng.chain_wgrad = rec["joint"], rec["two_streams"], rec["joint_streams"], rec["chain_wgrad"]
    eng.set_dropout(*(rec["drop"] or (0.0, 0.0, 0)))
    if rec["only"] == "fp16":
        eng.title.scaler.mult = rec["mult"]


def _run(eng, rec):
    """forward + backward of one record -> clones of what the rule compares.  Under a bucket hook each bucket's slice of flat_g is
    cloned when its hook fires and must equal what the slice holds after backward (the bucket was complete)."""
    s, t = _shared(), eng.title
    if rec["form"] == "tok":
        losses, score = eng.forward(*_feed(rec["feed"], "tok"))
    else:
        idx, y, bidx = _feed(rec["feed"], "idx")
        losses, score = eng.forward_indexed(s["title"], s["body"], idx, y, s["t_title"], s["t_body"],
                                            body_idx=bidx if rec["form"] == "idx_body" else None)
    assert eng.ran_joint == rec["joint"], (eng.ran_joint, rec)
    fired, snaps, ranges = [], [], eng.bucket_ranges()

    def hook(b):
        fired.append(b)
        snaps.append(t.flat_g[ranges[b][0]:ranges[b][1]].clone())
    eng.backward(after_bucket=hook if rec["hook"] else None)
    if rec["hook"]:
        assert fired == list(range(len(ranges))) and len(fired) >= 3, fired                 # every bucket once, in completion order
        for b, g in enumerate(snaps):
            assert torch.equal(g, t.flat_g[ranges[b][0]:ranges[b][1]]), "bucket %d changed after its hook fired" % b
    B = rec["B"]
    N, Rt = B * SR.C, B * SR.C + B
    assert eng.cur == (B, N, Rt) and t.B_alloc == eng.body.B_alloc == B and t.extra_rows == B * SR.LB and t.extra_seqs == B
    assert score.shape == (B, SR.C)
    # the masked LayerNorm-backward outputs (made by the first set_dropout that turns dropout on) are operands of the weight
    # gradients like every other per-token buffer: sized for this workspace, zero behind the rows of the pass that wrote them.  A
    # buffer kept across a re-lay would still give this step's bits at a smaller batch (the other operand's rows are zero there), so
    # the rule is held on the buffer itself
    rows_t, rows_b, rows_j = SR.rows(B)
    for e, m in ((t, rows_j if rec["joint"] else rows_t), (eng.body, rows_b)):
        assert (e.dyprem is None) == (e.dh1prem is None)
        for buf in (e.dyprem, e.dh1prem):
            assert buf is None or (buf.shape[0] == e.Mp and not bool(buf[m:].any())), "dropout buffer: %d rows for a workspace of %d, " \
                "or live rows behind row %d" % (buf.shape[0], e.Mp, m)
    return dict(losses=losses.clone(), score=score.clone(), S=t.S[:Rt].clone(), flat_g=t.flat_g.clone())


def _act(eng, act, ctx):
    """An action in front of a step (stage1_history_ref.step's `pre`)."""
    s, t, b = _shared(), eng.title, eng.body
    if act[0] == "encode_table":
        calls = (t.drop_calls, b.drop_calls)
        out = eng.encode_table(s[act[1]], act[1])
        assert (t.drop_calls, b.drop_calls) == calls                                       # a train=False pass: no call number ...
        assert out.shape == (SR.N_DOCS + 1, SR.D) and bool(torch.isfinite(out).all())
        if act[1] in ctx:                                                                  # ... no mask, and no trace of the steps before
            assert torch.equal(out, ctx[act[1]]), "encode_table(%s) differs from a fresh engine's" % act[1]
            ctx["encoded"] = ctx.get("encoded", 0) + 1
    elif act[0] == "step":
        assert b.sh is t.sh and b.sh_a1 is t.sh_a1 and b.sh_a1T is t.sh_a1T and b.scaler is t.scaler and b.flat_g is t.flat_g
        before = [{k: v.clone() for k, v in d.items()} for d in t.sh]
        a1, a1T = t.sh_a1.clone(), t.sh_a1T.clone()
        eng.step(act[1])
        if t.f16:
            t.scaler.drain(t)
        assert t.scaler.skipped == 0 and t.scaler.mult == 1.0
        torch.cuda.synchronize()
        for l, d in enumerate(before):                                                     # the update reached every 16-bit copy
            assert set(d) == {"qkv", "o", "w1", "w2", "qkvT", "oT", "w1T", "w2T"}
            for k, v in d.items():
                assert not torch.equal(v, t.sh[l][k]), (l, k)
                assert k.endswith("T") or torch.equal(t.sh[l][k].t(), t.sh[l][k + "T"]), (l, k)
        assert not torch.equal(a1, t.sh_a1) and not torch.equal(a1T, t.sh_a1T)
        assert torch.equal(t.sh_a1[:SR.Q].t(), t.sh_a1T[:, :SR.Q])
    else:
        raise ValueError(act)


def _play(dtype, schedule, eng, moving=False, after=None, ctx=None):
    """Drive `eng` through the schedule; every step against a fresh engine.  moving: the fresh engine takes the long-lived engine's
    weights as they are in front of the step (else the shared initial ones).  after(n, record, results, eng)."""
    s, ctx, n = _shared(), ctx if ctx is not None else {}, 0
    t, b = eng.title, eng.body
    for rec in SR.steps_for(schedule, dtype):
        for act in rec["pre"]:
            _act(eng, act, ctx)
        _set(eng, rec)
        calls, mult = (t.drop_calls, b.drop_calls), t.scaler.mult
        if moving and t.f16:
            t.scaler.drain(t)
        sd = eng.state_dict() if moving else s["P"]
        got = _run(eng, rec)
        k = 1 if rec["drop"] else 0
        assert (t.drop_calls, b.drop_calls) == (calls[0] + k, calls[1] + k)               # each pass numbers its own forward calls
        fresh = _engine(dtype, rec["B"])
        fresh.load_state_dict(sd)
        _set(fresh, rec)
        fresh.title.drop_calls, fresh.body.drop_calls = calls
        fresh.title.scaler.mult = mult
        want = _run(fresh, rec)
        torch.cuda.synchronize()
        n += 1
        assert bool(torch.isfinite(got["flat_g"]).all()) and float(got["flat_g"].abs().max()) > 0.0 and bool(torch.isfinite(got["losses"]).all())
        for k in WHAT:
            assert torch.equal(got[k], want[k]), "step %d (%s, B %d, %s, joint %s, hook %s, streams %s/%s, chain %s, drop %s, mult %g): %s " \
                "differs from the fresh engine's in %d elements, max |diff| %.3e" % (
                    n, rec["feed"], rec["B"], rec["form"], rec["joint"], rec["hook"], rec["two_streams"], rec["joint_streams"],
                    rec["chain_wgrad"], rec["drop"], t.scaler.mult, k, int((got[k] != want[k]).sum()),
                    float((got[k].double() - want[k].double()).abs().max()))
        if after is not None:
            after(n, rec, got, eng)
        del fresh, want
    return n


def _long_lived(dtype):
    assert E.AP_LONG == SR.AP_LONG
    eng = _engine(dtype, SR.B_FULL)
    eng.load_state_dict(_shared()["P"])
    assert eng.title.Lr == 32 and eng.body.Lr == 96 and eng.title.lo == 0 and eng.body.ap_ws is not None and eng.title.ap_ws is None
    return eng


def _eval_tables(eng):
    """encode_table of both tables on an engine that has run nothing yet."""
    s = _shared()
    return dict(title=eng.encode_table(s["title"], "title"), body=eng.encode_table(s["body"], "body"))


# ---------------------------------------------------------------------------------------------------------------- schedule A
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_schedule_a_every_step_equals_a_fresh_engine(dtype):
    """Fixed weights: joint -> joint + hook -> per pass -> per pass + hook (chained) -> joint -> SHORT joint (token feed; the oracle
    anchor) -> short per pass -> short joint + hook -> full (token feed) -> [encode_table x 2] per pass on one stream ->
    [encode_table x 2] joint with joint_streams -> per pass unchained -> per pass chained (body_idx given) -> fp16: that key at
    scaler.mult 0.5, then 1.0 -> the first step again -> fp16: the joint key at 0.5, then 1.0.
    The anchor against O.distill_fwd / O.distill_bwd: losses, scores and news vectors within 1e-3 (fp16) / 1.6e-2 (bf16) of
    max(1, |ref|), gradients 1.5e-2 / 6e-2 relative L2, no-op keys < 1e-3 absolutely, every other oracle norm >= 1e-7."""
    t0 = time.perf_counter()
    eng = _long_lived(dtype)
    ctx = _eval_tables(_long_lived(dtype))
    seen = {}

    def after(n, r, g, eng):
        seen[n] = g
        if not r["anchor"]:
            return
        assert n == 6
        out, G = SR.anchor_oracle()
        tol, l = TOL[dtype], g["losses"].cpu().numpy()
        for i, k in enumerate(("distill_loss", "target_loss", "emb_loss")):
            assert abs(l[i] - float(out[k])) <= tol * max(1.0, abs(float(out[k]))), (k, l[i], float(out[k]))
        sc, S = g["score"].cpu().numpy(), g["S"].cpu().numpy()
        N = r["B"] * SR.C
        se = np.abs(sc - out["student_score"]).max()
        assert se <= tol * max(1.0, np.abs(out["student_score"]).max())
        assert np.abs(S[:N].reshape(out["title_vec"].shape) - out["title_vec"]).max() <= tol * max(1.0, np.abs(out["title_vec"]).max())
        assert np.abs(S[N:] - out["body_vec"]).max() <= tol * max(1.0, np.abs(out["body_vec"]).max())
        assert set(eng.title.grads) == set(G)
        worst, wk = 0.0, ""
        for k in G:
            _, o, cnt, shp = eng.title.slot[k]
            got, ref = g["flat_g"][o:o + cnt].view(shp).cpu().numpy(), G[k]
            if k.endswith(W.NOOP):
                assert np.abs(got).max() < W.NOOP_ABS, k
                continue
            assert np.sqrt((ref.astype(np.float64) ** 2).sum()) >= W.MIN_NORM, k
            err = W.rel_l2(got, ref)
            if err > worst:
                worst, wk = err, k
            assert err < GTOL[dtype], "%s: relative L2 error %.3e" % (k, err)
        print("\n[stage1 history A %s] anchor, step 6 (%d + %d rows): score max|err| %.2e worst gradient %.2e (%s)" % (
            dtype, SR.rows(r["B"])[0], SR.rows(r["B"])[1], se, worst, wk[-48:]))

    n = _play(dtype, SR.SCHEDULE_A, eng, after=after, ctx=ctx)
    assert n == len(SR.SCHEDULE_A) - (4 if dtype == "bf16" else 0) and 6 in seen and ctx["encoded"] == 4
    assert eng.title.B_alloc == SR.B_FULL and eng.title.scaler.mult == 1.0 and eng.title.scaler.skipped == 0
    assert all(torch.equal(seen[1][k], seen[n][k]) for k in WHAT)                 # the first step again: the first step's bits
    assert not torch.equal(seen[1]["flat_g"], seen[2]["flat_g"])
    torch.cuda.synchronize()
    print("[stage1 history A %s] %d steps, each against a fresh engine: %.2f s" % (dtype, n, time.perf_counter() - t0))


# ---------------------------------------------------------------------------------------------------------------- schedule B
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_schedule_b_dropout_toggled_on_one_engine(dtype):
    """Dropout off -> on (0.1 / 0.1), joint -> on at the short batch, joint -> on, per pass -> [encode_table x 2, dropout set: no call
    number on either engine, the eval result] on, joint -> off.  The fresh engine gets set_dropout(...) and BOTH passes' call numbers.
    In the middle (behind the third step) load_optimizer_state_dict with a scalar dropout_calls is refused and changes nothing: the
    steps behind it still equal a fresh engine's."""
    t0 = time.perf_counter()
    eng = _long_lived(dtype)
    ctx = _eval_tables(eng)
    res = {}

    def after(n, r, g, eng):
        res[n] = g
        if n != 3:
            return
        t, b = eng.title, eng.body
        osd = eng.optimizer_state_dict()
        assert osd["dropout_calls"] == [2, 2]
        keep = (t.drop_calls, b.drop_calls, t.step_count, t.scaler.mult, t.adam_m.clone())
        with pytest.raises(ValueError, match="pair"):
            eng.load_optimizer_state_dict(dict(osd, dropout_calls=2))
        assert (t.drop_calls, b.drop_calls, t.step_count, t.scaler.mult) == keep[:4] and torch.equal(t.adam_m, keep[4])

    n = _play(dtype, SR.SCHEDULE_B, eng, ctx=ctx, after=after)
    assert n == 6 and eng.title.drop is None and eng.body.drop is None and (eng.title.drop_calls, eng.body.drop_calls) == (4, 4)
    assert ctx["encoded"] == 2
    assert not torch.equal(res[1]["losses"], res[2]["losses"])                   # the masks are live
    assert all(torch.equal(res[1][k], res[6][k]) for k in WHAT)                  # off again: the first step's bits
    torch.cuda.synchronize()
    print("\n[stage1 history B %s] %d steps: %.2f s" % (dtype, n, time.perf_counter() - t0))


# ---------------------------------------------------------------------------------------------------------------- schedule C
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_schedule_c_weights_move_between_unlike_steps(dtype):
    """joint -> step(lr) -> short per pass -> step(lr) -> joint + hook -> step(lr) -> joint; the fresh engine is loaded from
    state_dict() in front of each forward, so the 16-bit copies and their transposes, which the two engines share, are held to a
    rebuild from the fp32 weights.  After every update: each copy of both layers and the pooling head changed, each transposed
    copy equals its partner, the overflow guard skipped nothing."""
    t0 = time.perf_counter()
    eng = _long_lived(dtype)
    n = _play(dtype, SR.SCHEDULE_C, eng, moving=True)
    assert n == 4 and eng.title.step_count == 3 and eng.title.scaler.skipped == 0
    p0 = _shared()["P"]
    for k in (E.BERT + "encoder.layer.0.output.dense.weight", E.BERT + "encoder.layer.1.output.dense.weight", E.PFX + "dense.weight"):
        assert not torch.equal(eng.title.p(k), p0[k]), k
    frozen = E.BERT + "embeddings.word_embeddings.weight"
    assert torch.equal(eng.title.p(frozen), p0[frozen])
    torch.cuda.synchronize()
    print("\n[stage1 history C %s] %d steps, 3 updates: %.2f s" % (dtype, n, time.perf_counter() - t0))
