"""GPU: a training step does not depend on the steps before it.

One long-lived Engine is driven through the schedules of tests/history_ref.py (pinned by tests/test_history_ref_cpu.py): plans that
grow and shrink, two plans under one recorded key, the short batch and the way back, a bucket hook on and off, both feed forms, the
forward-only paths and the frozen-layer cache between steps, an accumulation window of unlike micro-batches, a loss scale that
moves, dropout toggled, weights that move under the 16-bit copies.

The rule for every step: after forward + backward on the long-lived engine, a FRESH Engine of that step's batch size gets the same
weights, dropout site and call number and loss-scale multiplier and runs only that step (or only that accumulation window); the
losses, the scores, S[:Rt] and the whole flat_g must be torch.equal.  No tolerance: single steps of a fresh engine are pinned to
the oracle elsewhere (tests/test_encoder_widths_gpu.py) and the kernels sum in a fixed order, so any difference is a dependence
on history.  One step - the eighth of schedule A, the first at the short batch - is held to the numpy oracle as well, under the
bounds of tests/widths_ref.py, which anchors "old and fresh agree" to the reference."""
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import engine as E                                               # noqa: E402
import history_ref as HR                                         # noqa: E402
import variants_ref as V                                         # noqa: E402
import widths_ref as W                                           # noqa: E402

DEV = "cuda:0"
WORD = E.BERT + "embeddings.word_embeddings.weight"
WHAT = ("losses", "score", "S", "flat_g")
_DEV = {}                                                        # device copies of the shared inputs: made once, never modified


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _shared(model=None):
    """model: None = history_ref's model and weights, else a variant of tests/variants_ref.py (the feeds and tables are the same)."""
    if "comb" not in _DEV:
        _DEV.update(comb=_t(HR.news()), tables=_t(HR.teachers()))
    if ("P", model) not in _DEV:
        _DEV["P", model] = {k: _t(v) for k, v in (HR.weights() if model is None else V.weights(model)).items()}
    return dict(comb=_DEV["comb"], tables=_DEV["tables"], P=_DEV["P", model])


def _feed(fid, form):
    if (fid, form) not in _DEV:
        if form == "idx":
            _DEV[fid, form] = tuple(_t(x) for x in HR.feed(fid))
        else:
            hist, m, cand, y, th, tc = HR.tokens(fid)
            _DEV[fid, form] = (_t(hist), _t(m), _t(cand), _t(y), [_t(x) for x in th], [_t(x) for x in tc])
    return _DEV[fid, form]


def _engine(dtype, B, model=None, **more):
    kw = HR.engine_kwargs() if model is None else V.engine_kwargs(model)
    return E.Engine(E.EngineConfig(**kw, **more), DEV, max_batch=B, dtype=dtype)


def _set(eng, rec):
    eng.set_dropout(*(rec["drop"] or (0.0, 0.0, 0)))
    if rec["only"] == "fp16":
        eng.scaler.mult = rec["mult"]


def _run(eng, rec, plan=None, snap=False):
    """forward + backward of one record -> clones of what the rule compares.  snap: under a bucket hook, each bucket's slice of
    flat_g is cloned when its hook fires and must equal what the slice holds after backward (the bucket was complete)."""
    s = _shared()
    if plan is None and rec["plan"]:
        plan = HR.plan(rec["feed"]).to(DEV)
    if rec["form"] == "idx":
        h, m, c, y = _feed(rec["feed"], "idx")
        losses, score = eng.forward_indexed(s["comb"], h, m, c, y, s["tables"], plan=plan)
    else:
        hist, m, cand, y, th, tc = _feed(rec["feed"], "tok")
        losses, score = eng.forward(hist, m, cand, y, th, tc, plan=plan)
    fired, snaps, ranges = [], [], eng.bucket_ranges()

    def hook(b):
        fired.append(b)
        if snap:
            snaps.append(eng.flat_g[ranges[b][0]:ranges[b][1]].clone())
    eng.backward(after_bucket=hook if rec["hook"] else None, micro=rec["micro"])
    if rec["hook"]:
        assert fired == list(range(len(eng.bucket_ranges()))) and len(fired) >= 3, fired     # every bucket, in completion order
        for b, g in enumerate(snaps):
            assert torch.equal(g, eng.flat_g[ranges[b][0]:ranges[b][1]]), "bucket %d changed after its hook fired" % b
    Rt = rec["B"] * (HR.U + HR.C + 1)
    assert eng.cur == (rec["B"], Rt - rec["B"], Rt)
    return dict(losses=losses.clone(), score=score.clone(), S=eng.S[:Rt].clone(), flat_g=eng.flat_g.clone())


def _act(eng, act, ctx):
    """An action in front of a step (history_ref.step's `pre`)."""
    s = _shared()
    if act[0] == "encode_news":
        ctx["ns"] = eng.encode_news(s["comb"])
        assert ctx["ns"].shape == (HR.N_NEWS + 1, HR.D) and (HR.N_NEWS + 1) % eng.N_alloc != 0
    elif act[0] == "user_vectors":
        h, m, _, _ = _feed(act[1], "idx")
        uv = eng.user_vectors(ctx["ns"], h, m)
        # pad_doc stands in for a masked history ; under user_log_mask nothing does: the pooling's weights are all masked
        assert bool(torch.isfinite(uv).all()) and (float(uv[1].abs().max()) > 0.0) != bool(eng.cfg.user_log_mask)
    elif act[0] == "encode_news_eval":
        calls = eng.drop_calls
        ns = eng.encode_news(s["comb"])
        assert eng.drop is not None and eng.drop_calls == calls                            # no call number ...
        assert torch.equal(ns, ctx["ns0"])                                                 # ... and no mask
    elif act[0] == "build_frozen_cache":
        ok = eng.build_frozen_cache(s["comb"])
        assert ok == (not eng.cfg.train_embeddings) and (eng.fcache is not None) == ok
    elif act[0] == "step":
        tr = {k: v.clone() for k, v in eng.sh[1].items()}
        a1, a1T, frozen = eng.sh_a1.clone(), eng.sh_a1T.clone(), {k: v.clone() for k, v in eng.sh[0].items()}
        eng.step(act[1])
        if eng.f16:
            eng.scaler.drain(eng)
            assert eng.scaler.skipped == 0 and eng.scaler.mult == 1.0
        torch.cuda.synchronize()
        assert set(tr) == {"qkv", "o", "w1", "w2", "qkvT", "oT", "w1T", "w2T"}
        for k, v in tr.items():                                                            # the update reached every 16-bit copy
            assert not torch.equal(v, eng.sh[1][k]), k
            assert k.endswith("T") or torch.equal(eng.sh[1][k].t(), eng.sh[1][k + "T"]), k
        assert not torch.equal(a1, eng.sh_a1) and not torch.equal(a1T, eng.sh_a1T)
        assert all(torch.equal(v, eng.sh[0][k]) for k, v in frozen.items())
    else:
        raise ValueError(act)


def _play(dtype, schedule, eng, moving=False, after=None, ctx=None, model=None, snap=False, **more):
    """Drive `eng` through the schedule; every step (accumulation window) against a fresh engine.  moving: the fresh engine takes
    the long-lived engine's weights as they are in front of the step (else the shared initial ones).  after(n, window, results).
    model, snap: as in _shared and _run."""
    s, ctx, n = _shared(model), ctx if ctx is not None else {}, 0
    for win in HR.windows(schedule, dtype):
        for act in win[0]["pre"]:
            _act(eng, act, ctx)
        _set(eng, win[0])
        calls, mult = eng.drop_calls, eng.scaler.mult
        if moving and eng.f16:
            eng.scaler.drain(eng)
        sd = eng.state_dict() if moving else s["P"]
        got = [_run(eng, r, snap=snap) for r in win]
        assert eng.drop_calls == calls + (len(win) if win[0]["drop"] else 0)
        fresh = _engine(dtype, win[0]["B"], model, **more)
        fresh.load_state_dict(sd)
        _set(fresh, win[0])
        fresh.drop_calls, fresh.scaler.mult = calls, mult
        want = [_run(fresh, r, snap=snap) for r in win]
        torch.cuda.synchronize()
        for r, g, w in zip(win, got, want):
            n += 1
            assert bool(torch.isfinite(g["flat_g"]).all()) and float(g["flat_g"].abs().max()) > 0.0 and bool(torch.isfinite(g["losses"]).all())
            for k in WHAT:
                assert torch.equal(g[k], w[k]), "step %d (%s, B %d, plan %s, %s, hook %s, micro %s, drop %s, mult %g): %s differs from " \
                    "the fresh engine's in %d elements, max |diff| %.3e" % (
                        n, r["feed"], r["B"], r["plan"], r["form"], r["hook"], r["micro"], r["drop"], eng.scaler.mult, k,
                        int((g[k] != w[k]).sum()), float((g[k].double() - w[k].double()).abs().max()))
            if after is not None:
                after(n, r, g, eng)
        del fresh, want
    return n


# ---------------------------------------------------------------------------------------------------------------- schedule A
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_schedule_a_every_step_equals_a_fresh_engine(dtype):
    """Fixed weights: plain -> plan 128 -> plan 64 -> [encode_news, user_vectors] plan 128' -> plan 64' -> plain + hook -> plain ->
    SHORT (token feed; the oracle anchor) -> short plan 64 -> short -> full (token feed) -> [build_frozen_cache] plan 64 -> plain +
    hook -> window (plan 128, plan 64) -> plain + hook; fp16: the same key at scaler.mult 0.5, then 1.0.
    The anchor against O.model_fwd / O.model_bwd under widths_ref.TOLS (fp16: loss 2e-3, score 3e-3 of max(1, |ref|), gradients
    2e-2 relative L2; bf16: 1.6e-2, 2.4e-2, 8e-2), no-op keys < 1e-3 absolutely, every other oracle norm >= 1e-7."""
    t0 = time.perf_counter()
    eng = _engine(dtype, HR.B_FULL)
    eng.load_state_dict(_shared()["P"])
    seen = {}

    def after(n, r, g, eng):
        seen[n] = g if r["anchor"] or r["only"] or n == 1 else None
        if not r["anchor"]:
            return
        assert n == 8
        ref_l, ref_s, G = HR.anchor_oracle()
        ltol, stol, gtol = W.TOLS[dtype]
        le = np.abs(g["losses"][:3].cpu().numpy() - ref_l).max() / max(1.0, np.abs(ref_l).max())
        se = np.abs(g["score"].cpu().numpy() - ref_s).max() / max(1.0, np.abs(ref_s).max())
        assert set(eng.grads) == set(G)
        worst, wk = 0.0, ""
        for k in G:
            _, o, cnt, shp = eng.slot[k]
            got, ref = g["flat_g"][o:o + cnt].view(shp).cpu().numpy(), G[k]
            if k.endswith(W.NOOP):
                assert np.abs(got).max() < W.NOOP_ABS, k
                continue
            assert np.sqrt((ref.astype(np.float64) ** 2).sum()) >= W.MIN_NORM, k
            err = W.rel_l2(got, ref)
            if err > worst:
                worst, wk = err, k
            assert err < gtol, "%s: relative L2 error %.3e" % (k, err)
        print("\n[history A %s] anchor, step 8 (%d rows): loss %.2e score %.2e worst gradient %.2e (%s)" % (
            dtype, HR.rows(r["B"]), le, se, worst, wk[-48:]))
        assert le < ltol and se < stol and np.isfinite(le + se + worst)

    n = _play(dtype, HR.SCHEDULE_A, eng, after=after)
    assert n == len(HR.SCHEDULE_A) - (2 if dtype == "bf16" else 0) and 8 in seen
    assert eng.fcache is not None and eng.B_alloc == HR.B_FULL and eng._clip_owner._acc_held == 0
    if dtype == "fp16":                                   # back at scale 1 on the first step's feed: the first step's bits
        assert eng.scaler.mult == 1.0 and all(torch.equal(seen[1][k], seen[n][k]) for k in WHAT)
    torch.cuda.synchronize()
    print("[history A %s] %d steps, each against a fresh engine: %.2f s" % (dtype, n, time.perf_counter() - t0))


# ---------------------------------------------------------------------------------------------------------------- schedule B
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_schedule_b_dropout_toggled_on_one_engine(dtype):
    """Dropout off -> on (0.1 / 0.1) -> on at the short batch -> [encode_news, train=False: no call number, no mask] on, plan 128 ->
    on -> off.  The fresh engine gets set_dropout(...) and the long-lived engine's call number."""
    t0 = time.perf_counter()
    eng = _engine(dtype, HR.B_FULL)
    eng.load_state_dict(_shared()["P"])
    ctx = dict(ns0=eng.encode_news(_shared()["comb"]))
    res = {}
    n = _play(dtype, HR.SCHEDULE_B, eng, ctx=ctx, after=lambda n, r, g, eng: res.__setitem__(n, g))
    assert n == 6 and eng.drop is None and eng.drop_calls == 4
    assert not torch.equal(res[1]["losses"], res[2]["losses"])                   # the masks are live
    assert all(torch.equal(res[1][k], res[6][k]) for k in WHAT)                  # off again: the first step's bits
    torch.cuda.synchronize()
    print("\n[history B %s] %d steps: %.2f s" % (dtype, n, time.perf_counter() - t0))


# ---------------------------------------------------------------------------------------------------------------- schedule C
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("embed", [False, True])
def test_schedule_c_weights_move_between_unlike_steps(dtype, embed):
    """[build_frozen_cache] plan 128 -> step(lr) -> short -> step(lr) -> plain -> step(lr) -> plan 64; the fresh engine is loaded
    from state_dict() in front of each forward, so refresh_shadows (the transposed copies and sh_a1T included), the rel-pos
    table and the cache of the frozen layer are held to a rebuild from the fp32 weights.  embed: train_embeddings=True - every
    layer keeps its activations, the cache is refused, and the word-table gradient is zero on every row the step does not name,
    the rows the step before named among them."""
    t0 = time.perf_counter()
    more = dict(train_embeddings=True) if embed else {}
    eng = _engine(dtype, HR.B_FULL, **more)
    eng.load_state_dict(_shared()["P"])
    assert eng.lo == (0 if embed else 1)
    named = []

    def after(n, r, g, eng):
        if not embed:
            assert eng.fcache is not None
            return
        assert eng.fcache is None
        _, o, cnt, shp = eng.slot[WORD]
        gw = g["flat_g"][o:o + cnt].view(shp)
        cur = HR.named_tokens(r)
        rest = torch.ones(shp[0], dtype=torch.bool, device=DEV)
        rest[torch.from_numpy(cur).to(DEV)] = False
        assert bool(rest[0]) and float(gw[rest].abs().max()) == 0.0 and float(gw[~rest].abs().max(1).values.min()) > 0.0
        if named:
            gone = np.setdiff1d(named[-1], cur)
            assert gone.size > 50 and float(gw[torch.from_numpy(gone).to(DEV)].abs().max()) == 0.0
        named.append(cur)

    n = _play(dtype, HR.SCHEDULE_C, eng, moving=True, after=after, **more)
    assert n == 4 and eng.step_count == 3 and len(named) == (4 if embed else 0)
    p0 = _shared()["P"]
    moved = E.BERT + "encoder.layer.1.output.dense.weight"
    assert not torch.equal(eng.p(moved), p0[moved]) and torch.equal(eng.p(WORD), p0[WORD]) != embed
    torch.cuda.synchronize()
    print("\n[history C %s embed %d] %d steps, 3 updates: %.2f s" % (dtype, embed, n, time.perf_counter() - t0))


# ---------------------------------------------------------------------------------------------------------------- the 64-row rule
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_a_plan_off_the_64_row_rule_is_refused(dtype):
    """build_plan(..., quantum=16) at L = 17: 48 sequences, 816 token rows, 816 % 64 = 48 - the weight gradients would read 16 rows
    of the pass before.  Engine.forward refuses it in both feed forms before anything is launched or re-laid; a plan for another
    batch size as well; the default plan of the same feed runs, and equals a fresh engine's step."""
    s = _shared()
    eng = _engine(dtype, HR.B_FULL)
    eng.load_state_dict(s["P"])
    _run(eng, HR.step("full_a"))                                          # live rows everywhere behind row 816
    q = HR.plan("q16", quantum=16)
    assert q.n_enc == 48 and (q.n_enc * HR.L) % 64 == 48
    keep = [x.clone() for x in (eng.X, eng.S, eng.Sv, eng.x0, eng.losses, eng.flat_g)]
    rec = HR.step("q16", plan=True)
    for form in ("idx", "tok"):
        with pytest.raises(ValueError, match="not a multiple of 64"):
            _run(eng, dict(rec, form=form), plan=q.to(DEV))
    with pytest.raises(ValueError, match="slots"):
        _run(eng, rec, plan=HR.plan("short_p64").to(DEV))
    with pytest.raises(ValueError, match="slots"):                       # ... nor does a short batch re-lay the workspace first
        _run(eng, HR.step("short_a"), plan=HR.plan("p64_a").to(DEV))
    torch.cuda.synchronize()
    assert eng.B_alloc == HR.B_FULL and all(torch.equal(a, b) for a, b in zip(keep, (eng.X, eng.S, eng.Sv, eng.x0, eng.losses, eng.flat_g)))
    assert _play(dtype, [rec, dict(rec, form="tok")], eng) == 2            # quantum 64: 64 x 17 rows
