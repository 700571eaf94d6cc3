"""GPU: in-batch negatives (Engine.forward(inbatch_ids=...)) in every step form, both 16-bit types.

The schedules of tests/inbatch_steps_ref.py (pinned by tests/test_inbatch_steps_ref_cpu.py) on one long-lived engine: the option on,
off and on again, a forward that no backward follows in front of a step of the other kind, forward-only paths inside an on step,
the short batch under a plan and the way back, both feed forms, dropout toggled, accumulation windows whose micro-batches differ in
the switch, weights that move, a loss scale that moves.  The rule is tests/test_step_history_gpu.py's: a FRESH engine of that
step's batch size gets the long-lived engine's weights, dropout site and call number and loss-scale multiplier and runs only that
step; losses, scores, eligible counts and the whole flat_g must be torch.equal.  A window's flat_g is the fp32 sum of the two
fresh backwards.

Then: the fp16 loss scale (a moved scale against autograd, an overflow in an on step and in an on window), the loss held to
inbatch_ref.loss on the engine's OWN rows (needs no port of NRMS or dropout), cls pooling and trainable embeddings against torch
autograd, the bucket hooks.  Bounds: widths_ref.TOLS, tests/test_embed_train_gpu.py's GTOL for the embedding keys, the kernel
tests' FWD on the mean loss; everything else is bit equality.

A forward-only path between an on step's forward and its backward: rank_metrics touches nothing of the engine, so the backward
follows it directly.  encode_news and user_vectors run through the step's own workspace (activations, dS, the score buffer) - a
backward behind them is lost with the option off as well - so there the forward runs again behind the path, and what is asserted
of the path itself is that it leaves Engine._ib_on, Engine.cur and every in-batch buffer as they were."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import history_ref as HR                                         # noqa: E402
import inbatch_ref as R                                          # noqa: E402
import inbatch_steps_ref as SR                                   # noqa: E402
import variants_ref as V                                         # noqa: E402
import widths_ref as W                                           # noqa: E402
from dedup import build_plan                                     # noqa: E402
from test_embed_train_gpu import GTOL as EMBED_GTOL              # noqa: E402
from test_heads_kernels_gpu import FWD                           # noqa: E402
from test_inbatch_gpu import make, run, same, against_port, dfeed    # noqa: E402
from test_step_history_gpu import DEV, _shared                   # noqa: E402

KEYS = ("losses", "score", "count", "flat_g")
_PLAN = {}


def plan_of(name):
    if name not in _PLAN:
        h, c, _, _ = R.engine_feed(name)
        p = build_plan(h, c, quantum=64)
        assert p is not None and p.n_enc == 64
        _PLAN[name] = p.to(DEV)
    return _PLAN[name]


def _set(eng, r):
    eng.set_dropout(*(r["drop"] or (0.0, 0.0, 0)))
    if eng.f16:
        eng.scaler.mult = r["mult"]


def _forward(eng, r, model="att"):
    return run(eng, r["feed"], r["on"], plan=plan_of(r["feed"]) if r["plan"] else None, form=r["form"], model=model, backward=False)


def _ib_state(eng):
    return eng._ib_on, eng.cur, {k: v.clone() for k, v in eng._inbatch.items()}


def _path(eng, what, r, ctx):
    s = _shared("att")
    h, c, m, y = dfeed(r["feed"])
    if what == "encode_table":
        ctx["ns"] = eng.encode_news(s["comb"])
    elif what == "user_vectors":
        assert bool(torch.isfinite(eng.user_vectors(ctx["ns"], h, m)).all())
    else:
        B, N = eng.cur[0], eng.cur[1]
        cands = [x for x in R.engine_feed(r["feed"])[1]]
        labels = [(np.arange(HR.C) == int(t)).astype(np.int32) for t in R.engine_feed(r["feed"])[3]]
        acc, scores, _ = eng.rank_metrics(eng.S[N:N + B].clone(), ctx["ns"], cands, labels)
        assert bool(torch.isfinite(scores).all()) and bool(torch.isfinite(acc).all())


def _step(eng, r, ctx=None):
    """One record on `eng` -> clones of what the rule compares.  ctx: the long-lived engine's (its `mid` path runs)."""
    out = _forward(eng, r)
    if r["mid"] and ctx is not None:
        on, cur, bufs = _ib_state(eng)
        _path(eng, r["mid"], r, ctx)
        on2, cur2, bufs2 = _ib_state(eng)
        assert on and on2 and cur2 == cur and all(torch.equal(bufs[k], bufs2[k]) for k in bufs), r["mid"]
        if r["mid"] != "rank_metrics":                     # the path ran through the step's workspace: the forward again
            again = _forward(eng, r)
            assert not same(out, again, ("losses", "score", "count")), r["mid"]
    if r["backward"]:
        eng.backward(micro=r["micro"])
        out["flat_g"] = eng.flat_g.clone()
    return out


def _play(dtype, name):
    s = _shared("att")
    eng = make(dtype, 5)
    ctx, n = {}, 0
    for win in SR.windows(SR.SCHEDULES[name], dtype):
        for act in win[0]["pre"]:
            if act[0] == "encode_table":
                ctx["ns"] = eng.encode_news(s["comb"])
            else:
                before = eng.flat[True].clone()
                eng.step(act[1])
                if eng.f16:
                    eng.scaler.drain(eng)
                    assert eng.scaler.skipped == 0
                assert not torch.equal(before, eng.flat[True])
        _set(eng, win[0])
        calls = eng.drop_calls
        if eng.f16:
            eng.scaler.drain(eng)
        sd = eng.state_dict()
        got = [_step(eng, r, ctx) for r in win]
        want = []
        for r in win:                                      # every record on an engine of its own, outside any window
            fresh = make(dtype, r["B"])
            fresh.load_state_dict(sd)
            _set(fresh, r)
            fresh.drop_calls = calls
            want.append(_step(fresh, dict(r, micro=None)))
            calls += 1 if r["drop"] else 0
            del fresh
        torch.cuda.synchronize()
        if len(win) == 2:                                  # the window: ((g0) + g1), one fp32 add per element
            want[1]["flat_g"] = want[0]["flat_g"] + want[1]["flat_g"]
            assert eng._clip_owner._acc_held == 0
        for r, g, w in zip(win, got, want):
            n += 1
            assert ("count" in g) == r["on"]
            assert bool(torch.isfinite(g["losses"][:3]).all())
            keys = [k for k in KEYS if k in w]
            assert set(g) == set(w) and ("flat_g" in g) == r["backward"]
            assert not same(g, w, keys), "%s step %d (%s, on %s, B %d, plan %s, %s, micro %s, drop %s, mult %g, mid %s): %s differ" % (
                name, n, r["feed"], r["on"], r["B"], r["plan"], r["form"], r["micro"], r["drop"], r["mult"], r["mid"], same(g, w, keys))
            if r["on"]:
                h, c, _, _ = R.engine_feed(r["feed"])
                assert (g["count"].cpu().numpy() == R.eligibility(h, c).sum(1)).all()
    return n, eng


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("name", ["toggle", "paths", "moving"])
def test_schedule_every_step_equals_a_fresh_engine(dtype, name):
    n, eng = _play(dtype, name)
    assert n == len(SR.SCHEDULES[name])
    if name == "moving":
        assert eng.step_count == 2 and eng.drop is None and eng.drop_calls == 2


# ---------------------------------------------------------------------------------------------------------------- fp16 loss scale
def test_the_loss_scale_moves_under_on_steps():
    """scaler.mult 1 -> 0.5 -> 2 -> 1 on one engine, every step on: each equals a fresh engine at that multiplier."""
    n, eng = _play("fp16", "scale")
    assert n == 4 and eng.scaler.mult == 1.0


def test_a_moved_scale_against_autograd():
    """the gradient of the new term is unscaled fp32 like all the heads', the loss scale enters below it.
    The whole step at multiplier 0.5 under the bounds it meets at 1.0."""
    against_port("fp16", "att", "e5", True, mult=0.5)


def _state(eng):
    return [x.clone() for x in (eng.flat[True], eng.adam_m, eng.adam_v, eng.adam_vmax)]


@pytest.mark.parametrize("window", [False, True])
def test_an_overflow_in_an_on_step_skips_one_update(window):
    """An inf in flat_g behind an on backward (window: in the accumulator behind the first micro-batch of two, both on): the update
    is skipped as one step - parameters and all three moment buffers keep their bits, scaler.skipped == 1 - and the next on step
    equals a fresh engine's at the halved scale."""
    eng = make("fp16", 5)
    if window:
        run(eng, "e5", True, micro=(0, 2))
        eng._acc[eng.n_train // 2] = float("inf")          # as if micro-batch 0's backward had overflowed
        run(eng, "e5b", True, micro=(1, 2))
    else:
        run(eng, "e5", True)
        eng.flat_g[eng.n_train // 2] = float("inf")
    assert not bool(torch.isfinite(eng.flat_g).all())
    before = _state(eng)
    eng.step(1e-3, grad_scale=0.5 if window else 1.0)
    eng.scaler.drain(eng)
    assert all(torch.equal(a, b) for a, b in zip(before, _state(eng)))
    assert eng.scaler.skipped == 1 and eng.step_count == 0 and eng.scaler.mult == 0.5 and eng._clip_owner._acc_held == 0
    got = run(eng, "e5b", True)
    fresh = make("fp16", 5)
    fresh.scaler.mult = 0.5
    want = run(fresh, "e5b", True)
    torch.cuda.synchronize()
    assert not same(got, want, KEYS) and bool(torch.isfinite(got["flat_g"]).all())
    eng.step(1e-3)
    eng.scaler.drain(eng)
    assert eng.scaler.skipped == 1 and eng.step_count == 1 and not torch.equal(before[0], eng.flat[True])


# ---------------------------------------------------------------------------------------------------------------- own rows
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("model,drop,plan", [("att", SR.DROP, False), ("cls_nrms", None, False), ("att_nrms_ulm", None, False),
                                             ("att", None, True), ("att_nrms_ulm", SR.DROP, True)])
def test_the_loss_on_the_engines_own_rows(dtype, model, drop, plan):
    """Conditional on what the engine itself computed - eng.S's user and candidate rows, eng.score, the labels, the plan's words -
    losses[1] is inbatch_ref.loss in float64 within the kernel tests' bound on the mean loss; the words and the counts are
    inbatch_ref.eligibility's.  Under dropout, the NRMS user encoders and a de-duplication plan, none of which the port has."""
    B, U, C = 5, HR.U, HR.C
    eng = make(dtype, B, model)
    if drop:
        eng.set_dropout(*drop)
    got = run(eng, "e5", True, plan=plan_of("e5") if plan else None, model=model, backward=False)
    N = B * (U + C)
    S, score, label = eng.S[:N + B].cpu().numpy(), eng.score[:B].cpu().numpy(), eng.label.cpu().numpy()
    words = eng._inbatch["elig"].cpu().numpy().view(np.uint32)
    h, c, _, y = R.engine_feed("e5")
    E = R.eligibility(h, c)
    assert (words == R.words(E)).all() and (got["count"].cpu().numpy() == E.sum(1)).all() and (label == y).all()
    assert (score == got["score"].cpu().numpy()).all() and np.isfinite(S).all()
    ref = R.loss(S[N:], S[B * U:N], score, label, E, eng.cfg.coef)
    err = abs(float(got["losses"][1]) - ref["target"])
    print("\n[inbatch own rows %s %s drop %s plan %s] target %.5f, err / bound %.3f" % (
        dtype, model, bool(drop), plan, ref["target"], err / (FWD * abs(ref["target"]))))
    assert err <= FWD * abs(ref["target"])
    if drop:                                               # the masks are live: another call number, other rows
        other = run(eng, "e5", True, plan=plan_of("e5") if plan else None, model=model, backward=False)
        assert not torch.equal(other["losses"], got["losses"]) and torch.equal(other["count"], got["count"])


# ---------------------------------------------------------------------------------------------------------------- autograd
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_cls_pooling_against_autograd(dtype):
    """variants_ref's cls_add: cls pooling, the additive user encoder (the port follows both)."""
    against_port(dtype, "cls_add", "e5", True)


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("model", ["att", "cls_add"])
def test_trainable_embeddings_against_autograd(dtype, model):
    """train_embeddings=True: the five embedding keys as well, to tests/test_embed_train_gpu.py's bound."""
    against_port(dtype, model, "e5", True, embed_gtol=EMBED_GTOL[dtype])


# ---------------------------------------------------------------------------------------------------------------- bucket hooks
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("model", ["att", "cls_nrms"])
def test_bucket_hooks(dtype, model):
    """An on backward with after_bucket: every bucket is complete when its hook fires (its snapshot is that range of the final
    flat_g), and the final flat_g is the backward's without a hook."""
    plain = run(make(dtype, 5, model), "e5", True, model=model)
    eng = make(dtype, 5, model)
    run(eng, "e5", True, model=model, backward=False)
    ranges, fired, snaps = eng.bucket_ranges(), [], []

    def hook(b):
        fired.append(b)
        snaps.append(eng.flat_g[ranges[b][0]:ranges[b][1]].clone())
    eng.backward(after_bucket=hook)
    torch.cuda.synchronize()
    assert fired == list(range(len(ranges))) and len(fired) >= 3
    for b, g in enumerate(snaps):
        assert torch.equal(g, eng.flat_g[ranges[b][0]:ranges[b][1]]), "bucket %d changed after its hook fired" % b
    assert torch.equal(eng.flat_g, plain["flat_g"])


# ---------------------------------------------------------------------------------------------------------------- two ranks
def _ranks(tmp_path, mode, port, limit=300.0):
    """tests/workers/dp_rank.py once per rank over gloo, both on cuda:0 (tests/test_dp_gpu.py's _launch): a time limit per launch,
    a rank that is still running when the other has failed or the limit has passed is killed, and nothing is started after."""
    import os
    import subprocess
    import sys
    import time
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = str(tmp_path / (mode + "_rank%d.npz"))
    procs, logs, t0 = [], [], time.time()
    for r in range(2):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE="2", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        logs.append(open(str(tmp_path / ("%s_rank%d.log" % (mode, r))), "w"))
        procs.append(subprocess.Popen([sys.executable, os.path.join(root, "tests", "workers", "dp_rank.py"), out, "fp16", "10", "2", mode],
                                      env=env, stdout=logs[-1], stderr=subprocess.STDOUT))
    try:
        while any(p.poll() is None for p in procs) and all(p.poll() in (None, 0) for p in procs) and time.time() - t0 < limit:
            time.sleep(0.02)
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
            p.wait()
        for f in logs:
            f.close()
    for r, p in enumerate(procs):
        assert p.returncode == 0, "rank %d: status %s after %.0f s\n%s" % (
            r, p.returncode, time.time() - t0, open(str(tmp_path / ("%s_rank%d.log" % (mode, r)))).read()[-3000:])
    return [np.load(out % r) for r in range(2)]


def test_two_ranks_each_against_its_own_half(tmp_path):
    """fp16 over gloo, rank 0 on e5 and rank 1 on e5b, two on steps with gs.launch the hook and step(sync=gs) the update.  A rank
    ranks against its own batch only: the reduced flat_g of step 1 is the fp32 mean of two single-process engines' flat_g, each on
    one half with the option on - torch.equal -, the counts are the reference's for the rank's own half, and both ranks end on
    identical parameters."""
    two = _ranks(tmp_path, "inbatch", 29651)
    g = [run(make("fp16", 5), name, True) for name in ("e5", "e5b")]
    want = ((g[0]["flat_g"] + g[1]["flat_g"]) * 0.5).cpu()
    for r, (z, name) in enumerate(zip(two, ("e5", "e5b"))):
        h, c, _, _ = R.engine_feed(name)
        assert float(z["scale"]) == 0.5 and int(z["skipped"]) == 0 and int(z["steps"]) == 2
        assert (z["counts"] == R.eligibility(h, c).sum(1)[None, :]).all() and z["counts"].shape == (2, 5)
        assert torch.equal(torch.from_numpy(z["grads"][0]), want), "rank %d: %d elements differ" % (r, int((z["grads"][0] != want.numpy()).sum()))
        assert torch.equal(torch.from_numpy(z["losses"][0]), g[r]["losses"].cpu())
        assert not np.array_equal(z["losses"][0], z["losses"][1]) and np.isfinite(z["grads"]).all()      # the first step moved the weights
    assert np.array_equal(two[0]["grads"], two[1]["grads"]) and np.array_equal(two[0]["params"], two[1]["params"])
    assert not np.array_equal(two[0]["counts"], two[1]["counts"]) and np.isfinite(two[0]["params"]).all()


# ---------------------------------------------------------------------------------------------------------------- run.py
import test_run_dp_resume_gpu as RD                              # noqa: E402
from test_run_dp_resume_gpu import base, filefed                # noqa: E402,F401 (module-scoped fixtures: the shards, made once)

FLAG = ["--inbatch_negatives", "True"]
_NEXT_PORT = [29959]                                             # 29960 and up; that file's own launches keep their numbering


def _abc(root, flags, world, only_a=False):
    """test_run_dp_resume_gpu.abc on this file's ports."""
    keep, RD._PORT[0] = RD._PORT[0], _NEXT_PORT[0]
    try:
        return RD.abc(root, flags, world, only_a=only_a)
    finally:
        _NEXT_PORT[0], RD._PORT[0] = RD._PORT[0], keep


def _said_counts(log, rank):
    import re
    return [float(x) for x in re.findall(r"\[%d\] in-batch negatives: ([0-9.]+) eligible per impression" % rank, log)]


@pytest.mark.parametrize("world", [1, 2])
def test_run_py_resumes_bit_for_bit_with_the_flag(base, world):
    """The A / B / C scheme of tests/test_run_dp_resume_gpu.py, synthetic, with --inbatch_negatives True and that file's ON flags
    (accumulation 2, clip, decay, schedule, average): C's epoch-2.pt equals A's in every bit, the ranks agree, the flag is recorded.
    World 1 then resumes B's epoch-1.pt once more WITHOUT the flag: the warning DESIGN.md promises, and the run trains on."""
    runs = _abc(base / ("inbatch_w%d" % world), RD.MODEL + RD.ON + RD.SYNTH + FLAG, world)
    if world == 2:
        for k in "ABC":
            RD.ranks_agree(runs[k], "in-batch, synthetic, world 2, " + k)
        for k in runs["A"].npz[1]:
            assert np.array_equal(runs["A"].npz[1][k], runs["C"].npz[1][k]), "rank 1: C differs from A in " + k
    a2 = RD.c_equals_a(runs, 6, world)
    assert a2["train_state"]["flags"]["inbatch_negatives"] is True
    RD.logs_of_a_resume(runs["C"])
    for r in range(world):
        n = _said_counts(runs["A"].logs[r], r)
        assert len(n) == 12 and all(0.0 < x <= 3 * 5 for x in n), n                      # --log_steps 1; B = 4, C = 5
    if world == 1:
        b1 = RD.load(runs["B"].dir, "epoch-1.pt")
        keep, RD._PORT[0] = RD._PORT[0], _NEXT_PORT[0]
        try:
            off = RD.launch(str(base / "inbatch_w1" / "D.out"), runs["B"].dir, RD.MODEL + RD.ON + RD.SYNTH + [
                "--save_optimizer", "True", "--epochs", "2", "--load_ckpt_name", "epoch-1.pt", "--resume", "True"], 1)
        finally:
            _NEXT_PORT[0], RD._PORT[0] = RD._PORT[0], keep
        log = off.logs[0]
        assert "--resume True: --inbatch_negatives is False, the run that wrote" in log and "had True" in log, log[-3000:]
        assert "continuing at epoch 1" in log and not _said_counts(log, 0)
        d2 = RD.load(runs["B"].dir, "epoch-2.pt")
        assert "inbatch_negatives" not in d2["train_state"]["flags"] and d2["train_state"]["epoch"] == 2
        assert d2["train_state"]["updates"] > b1["train_state"]["updates"]
        w = "student.news_encoder.dense.weight"
        assert not torch.equal(d2["model_state_dict"][w], a2["model_state_dict"][w])     # another loss from epoch 2 on
        assert bool(torch.isfinite(d2["model_state_dict"][w]).all())


def test_run_py_feed_forms_agree_with_the_flag(base, filefed):
    """File-fed, one rank, the three feed forms with the flag on (the resident feeds pass their indices, the reference feed its
    batches' decoded ids): two epochs each, every bit of the checkpoints equal."""
    got = {}
    for form in RD.FORMS:
        run_ = _abc(base / ("inbatch_filefed_" + form), filefed + FLAG + RD.FORMS[form], 1, only_a=True)["A"]
        got[form] = RD.load(run_.dir, "epoch-2.pt")
        assert got[form]["train_state"]["flags"]["inbatch_negatives"] is True
        assert form == "decode_process" or _said_counts(run_.logs[0], 0) or "in-batch negatives" in run_.logs[0]
    for form in ("producer_thread", "rows_from_host"):
        for key in RD.CKPT:
            RD._equal(got["decode_process"][key], got[form][key], "in-batch, decode_process against %s: %s" % (form, key))
