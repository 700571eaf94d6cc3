"""LAMB through the engine: Engine.step(lamb=True), trust_ratios(), Stage1Engine, two ranks, run.py --optimizer lamb.

The 2-layer, 2-teacher hashinit engine and the random-flat_g pattern of tests/test_grad_clip_gpu.py (its helpers are imported, as
tests/test_adamw_gpu.py imports them).  The reference is tests/lamb_ref.lamb_step in float64 on the engine's own slot table.  Every
step is checked against the float64 step FROM THE ENGINE'S OWN STATE before it (parameters, moments, average read back), so the
inputs of the two sides are the same bits and the derived bound of the trust ratios (lamb_ref.trust_rtol: the kernel's summation
order and the roundings of u) applies as it stands; no drift can hide between steps.  The other bounds are the optimiser tests' own
(p and the average rtol 1e-5 atol 1e-6; m, v, vmax rtol 1e-5 with a floor of 1e-5 of the buffer's largest magnitude).  The rates are
large on purpose (2e-2, 1e-2, 5e-3): hashinit weights have ||w|| / ||u|| far from 1, so the float64 AdamW step WITHOUT trust ratios
misses the engine's parameters by more than the bound in the adapted tensors - and in none of the exempt ones."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import adamw_ref as A                                   # noqa: E402
import lamb_ref as L                                    # noqa: E402
import tnr_hip as T                                     # noqa: E402
from test_heads_kernels_gpu import check, check_abs     # noqa: E402
from test_grad_clip_gpu import make, fill, gen, state, FakeSync, ROOT, DEV     # noqa: E402
from test_adamw_gpu import tables                       # noqa: E402

RATES = (2e-2, 1e-2, 5e-3)                              # lr, lr_bert, lr_news_head
WD, W, TD, GS = 0.01, 2, 5, 0.5
ON = dict(lamb=True, weight_decay=WD, warmup_steps=W, lr_decay_steps=TD)
RKW = dict(grad_scale=GS, lr_bert=RATES[1], lr_news_head=RATES[2])
f32 = L.f32


def snapshot(eng, ams, ema=False):
    """The buffers a step reads, as float64 on the host."""
    torch.cuda.synchronize()
    h = lambda t: t.cpu().numpy().astype(np.float64)
    own = eng._clip_owner
    return dict(p=h(eng.flat[True]), m=h(eng.adam_m), v=h(eng.adam_v), x=h(eng.adam_vmax) if ams else None,
                e=(h(own._ema) if own._ema is not None else h(eng.flat[True])) if ema else None)


def expected(eng, pre, gh, bc, mult, ams, rates=RATES, wd=WD, gs=GS, coef=None, ema_w=None):
    """One float64 LAMB step from `pre`: the rates of the three ranges x mult as the C floats the kernel gets, grad_scale x the
    DEVICE's clip coefficient as the kernel's fp32 product."""
    per_range, _ = tables(eng, rates)
    lr = np.zeros_like(per_range)
    for r in set(rates):
        lr[per_range == r] = f32(r * mult)
    g_eff = f32(gs) if coef is None else float(np.float32(gs) * np.float32(coef))
    p, m, v, x, info = L.lamb_step(L.slots(eng.slot), pre["p"], gh, pre["m"], pre["v"], pre["x"], bc, lr, f32(wd), f32(0.9), f32(0.999),
                                   f32(1e-8), grad_scale=g_eff)
    e = pre["e"] + f32(ema_w) * (p - pre["e"]) if ema_w is not None else None
    return dict(p=p, m=m, v=v, x=x, e=e, info=info)


def compare(what, eng, want, ams, trust=True):
    check_abs("%s/p" % what, eng.flat[True].cpu().numpy(), want["p"], 1e-5, 1e-6)
    check("%s/m" % what, eng.adam_m.cpu().numpy(), want["m"], 1e-5, 1e-5)
    check("%s/v" % what, eng.adam_v.cpu().numpy(), want["v"], 1e-5, 1e-5)
    if ams:
        check("%s/vmax" % what, eng.adam_vmax.cpu().numpy(), want["x"], 1e-5, 1e-5)
    else:
        assert float(eng.adam_vmax.abs().max()) == 0.0
    if want["e"] is not None:
        check_abs("%s/ema" % what, eng._clip_owner._ema.cpu().numpy(), want["e"], 1e-5, 1e-6)
    if trust:
        compare_trust(what, eng, want["info"])


def compare_trust(what, eng, info):
    got = eng.trust_ratios()
    adapted = [k for k, v in eng.slot.items() if v[0] and A.decays(k, v[3])]
    assert sorted(got) == sorted(adapted) and len(got) < sum(1 for v in eng.slot.values() if v[0])
    worst = 0.0
    for k in adapted:
        trust, wn, un, kappa = info[k]
        bound = L.trust_rtol(kappa)
        assert bound < 1e-5, (k, kappa)
        t, w_, u_ = got[k]
        assert abs(t - trust) <= bound * trust, (what, k, t, trust, bound)
        assert abs(w_ - wn) <= L.norm_rtol(1.0, of_u=False) * wn and abs(u_ - un) <= L.norm_rtol(kappa) * un, (what, k)
        worst = max(worst, abs(t - trust) / (bound * trust))
    ts = [v[0] for v in got.values()]
    print("[lamb] %s: %d adapted tensors, trust %.3g .. %.3g, worst err / bound %.3f" % (what, len(ts), min(ts), max(ts), worst))


def adam_misses_adapted_only(eng, pre, gh, bc, mult, ams, coef):
    """The float64 AdamW step (decoupled decay, no trust ratio) from the same state: off by more than the parameter bound in
    elements of adapted tensors, within it in every exempt one.  What belongs to no tensor (alignment gaps, the reserved rows behind
    att_fc1, where fill() leaves a random gradient) is no chunk's: LAMB leaves its bits, whatever Adam would do there."""
    lr, mask = tables(eng, RATES)
    g_eff = GS if coef is None else GS * coef
    plain = A.adamw_step(pre["p"], gh, pre["m"], pre["v"], pre["x"], bc, lr * mult, mask, WD, grad_scale=g_eff)[0]
    got = eng.flat[True].cpu().numpy().astype(np.float64)
    over = np.abs(got - plain) > 1e-6 + 1e-5 * np.abs(plain)
    covered = np.zeros(eng.n_train, bool)
    for _, o, n, _ in L.slots(eng.slot):
        covered[o:o + n] = True
    assert over[mask].mean() > 0.5 and not over[~mask & covered].any() and (~mask & covered).sum() > 1000
    assert (~covered).sum() >= 64 and (got[~covered] == pre["p"][~covered]).all()


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_off_is_the_step_as_it_was(monkeypatch, dtype):
    """Absent / None / False: the same C-ABI calls in the same order, the same bits, no table.  On: no tnr_amsgrad_step* /
    tnr_adamw_step* call, one norm pass, one commit, one apply launch per rate range."""
    calls = []
    real = T.call

    def recorder(name, *a):
        calls.append(name)
        return real(name, *a)
    monkeypatch.setattr(T, "call", recorder)
    for base in ({}, dict(weight_decay=WD, max_grad_norm=1.0, ema_decay=0.9)):
        outs, seqs = [], []
        for kw in ({}, dict(lamb=None), dict(lamb=False)):
            eng = make(dtype)
            g = gen()
            del calls[:]
            for step in range(2):
                fill(eng, g, 1e-3)
                eng.step(RATES[0], **RKW, **base, **kw)
            outs.append(state(eng))
            seqs.append(list(calls))
            assert eng._lamb_state is None and eng.trust_ratios() is None
        assert seqs[0] == seqs[1] == seqs[2] and any(n.startswith("tnr_amsgrad_step") or n.startswith("tnr_adamw_step") for n in seqs[0])
        assert not any("lamb" in n for n in seqs[0])
        for other in outs[1:]:
            assert all(torch.equal(a, b) for a, b in zip(outs[0], other))
        eng = make(dtype)
        fill(eng, gen(), 1e-3)
        del calls[:]
        eng.step(RATES[0], **RKW, **base, lamb=True)
        assert not any(n.startswith("tnr_amsgrad_step") or n.startswith("tnr_adamw_step") for n in calls), calls
        assert (calls.count("tnr_lamb_norms"), calls.count("tnr_lamb_commit"), calls.count("tnr_lamb_step")) == (1, 1, 3)
        assert eng._lamb_state is not None and eng._decay_map is None and eng.trust_ratios() is not None
        assert not torch.equal(state(eng)[0], outs[0][0])


@pytest.mark.parametrize("ema", [False, True])
@pytest.mark.parametrize("clipped", [False, True])
@pytest.mark.parametrize("dtype,ams", [("fp16", True), ("bf16", False)])
def test_three_steps_against_float64(dtype, ams, clipped, ema):
    """Three rate ranges, wd = 0.01, W = 2, T = 5 (multipliers 0, 1/2, 1), grad_scale 0.5; AMSGrad behind fp16's guard and plain Adam
    under bf16, with and without max_grad_norm (which clips the first step) and the average."""
    eng = make(dtype)
    max_norm = 0.6 * GS * 1e-3 * float(np.sqrt(eng.n_train))
    kw = dict(ON, **(dict(max_grad_norm=max_norm) if clipped else {}), **(dict(ema_decay=0.9) if ema else {}))
    p0 = eng.flat[True].clone()
    g, coefs = gen(), []
    for s, sc in enumerate((1e-3, 1e-4, 1e-3)):
        fill(eng, g, sc)
        gh = eng.flat_g.cpu().numpy()
        pre = snapshot(eng, ams, ema)
        eng.step(RATES[0], amsgrad=ams, **RKW, **kw)
        mult = A.schedule(s, W, TD)
        assert eng.lr_scale == mult == (0.0, 0.5, 1.0)[s]
        coef = eng.grad_norm()[1] if clipped else None
        coefs.append(coef)
        want = expected(eng, pre, gh, s + 1, mult, ams, coef=coef, ema_w=1.0 - 0.9 if ema else None)
        compare("engine lamb %s ams%d clip%d ema%d step%d" % (dtype, ams, clipped, ema, s + 1), eng, want, ams)
        if s == 0:
            assert torch.equal(eng.flat[True], p0)                           # the first update of a warmup has rate 0
            assert not ema or torch.equal(eng._ema, p0)
    if clipped:
        assert coefs[0] < 1.0 and coefs[1] == 1.0
    adam_misses_adapted_only(eng, pre, gh, 3, 1.0, ams, coef)
    assert eng._decay_map is None                                            # the coupled decay needs no bit map
    if dtype == "fp16":
        eng.scaler.drain(eng)
        assert eng.scaler.skipped == 0 and eng.step_count == 3


@pytest.mark.parametrize("clipped", [False, True])
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_bucketed_equals_whole(dtype, clipped):
    """A sync whose collectives are complete but pending: the step waits for every bucket in bucket_ranges() order (scanning each as
    it lands when clip or the guard is on), then runs the norm pass - bit-identical to the step without sync, trust table included."""
    outs, trusts = [], []
    for mode in ("whole", "bucketed"):
        eng = make(dtype)
        p0 = eng.flat[True].clone()
        g = gen()
        ranges = eng.bucket_ranges()
        kw = dict(ON, ema_decay=0.9, **(dict(max_grad_norm=0.6 * GS * 1e-3 * float(np.sqrt(eng.n_train))) if clipped else {}))
        for step in range(3):
            fill(eng, g, 1e-3)
            sync = FakeSync(ranges) if mode == "bucketed" else None
            eng.step(RATES[0], amsgrad=dtype == "fp16", sync=sync, **RKW, **kw)
            if sync is not None:
                assert sync.waited == list(range(len(ranges))) and not sync.pending
        outs.append(state(eng) + [eng._ema.clone(), eng._lamb_state.trust.clone()])
        trusts.append(eng.trust_ratios())
        if dtype == "fp16":
            eng.scaler.drain(eng)
            assert eng.scaler.skipped == 0
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(*outs))
    assert trusts[0] == trusts[1] and not torch.equal(outs[0][0], p0)


def test_fp16_skipped_step_moves_nothing_and_keeps_the_trust_table():
    """Six steps with W = 4 and an inf written into flat_g at the third: one skip.  Every other step is the float64 step with the
    bias corrections and the multiplier of the updates TAKEN (five in all: 0, 1/4, 2/4, 3/4, 1) - the step behind the skip runs before
    the host knows of it, and BOTH passes pick candidate 1 on the device.  The skipped step changes no bit, the trust table included."""
    eng = make("fp16")
    g, taken = gen(), 0
    for step in range(6):
        fill(eng, g, 1e-3)
        if step == 2:
            eng.flat_g[eng.n_train // 2 + 1] = float("inf")
        gh = eng.flat_g.cpu().numpy()
        before = state(eng)[:4] + ([eng._lamb_state.trust.clone()] if step else [])
        seen = eng.trust_ratios()
        pre = snapshot(eng, True)
        eng.step(RATES[0], **RKW, lamb=True, weight_decay=WD, warmup_steps=4)
        if step == 2:
            assert all(torch.equal(a, b) for a, b in zip(before, state(eng)[:4] + [eng._lamb_state.trust]))
            assert eng.trust_ratios() == seen and seen is not None
            continue
        mult = A.schedule(taken, 4, 0)
        taken += 1
        want = expected(eng, pre, gh, taken, mult, True)
        compare("engine lamb skip: step %d = update %d (x%.2f)" % (step + 1, taken, mult), eng, want, True)
    eng.scaler.drain(eng)
    assert eng.scaler.skipped == 1 and eng.step_count == 5 and int(eng.scaler.guard[1]) == 1 and taken == 5


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_accumulation_window_is_one_step_on_the_sum(dtype):
    """K = 2: two backwards into the window, then step(grad_scale / 2, lamb) == the same step on a flat_g filled with g0 + g1."""
    from test_grad_accum_gpu import make as make_acc, fwd
    kw = dict(lamb=True, weight_decay=WD, max_grad_norm=0.05, ema_decay=0.9, grad_scale=1.0 / 2.0, lr_bert=RATES[1], amsgrad=dtype == "fp16")
    eng = make_acc(dtype)
    gs = []
    for j in range(2):
        fwd(eng, 2 * j)
        eng.backward(micro=(j, 2))
        if j == 0:
            gs.append(eng._acc.clone())
    total = eng.flat_g.clone()
    eng.step(RATES[0], **kw)
    other = make_acc(dtype)
    other.flat_g.copy_(total)
    other.step(RATES[0], **kw)
    for a, b in zip(state(eng) + [eng._ema, eng._lamb_state.trust], state(other) + [other._ema, other._lamb_state.trust]):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert eng.trust_ratios() == other.trust_ratios() and not torch.equal(total, gs[0])
    assert not torch.equal(eng.flat[True], make_acc(dtype).flat[True])


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_resume_is_bit_exact(dtype):
    """Save after 2 updates, load into a fresh engine, 2 more == 4 uninterrupted, on every buffer; the state's format is unchanged
    (no new key, no trust table)."""
    straight = make(dtype)
    kw = dict(ON, ema_decay=0.9, max_grad_norm=0.6 * GS * 1e-3 * float(np.sqrt(straight.n_train)), amsgrad=dtype == "fp16", **RKW)
    g = gen()
    grads = []
    for s in range(4):
        fill(straight, g, 1e-3)
        grads.append(straight.flat_g.clone())
        straight.step(RATES[0], **kw)
    first = make(dtype)
    for s in range(2):
        first.flat_g.copy_(grads[s])
        first.step(RATES[0], **kw)
    sd, esd, osd = first.state_dict(), first.ema_state_dict(), first.optimizer_state_dict()
    import optstate
    assert sorted(osd) == sorted(optstate.make(dtype, 0, {})) and osd["format"] == optstate.FORMAT == 1 and osd["step"] == 2
    assert all(sorted(v) == sorted(optstate.MOMENTS) for v in osd["state"].values())
    second = make(dtype)
    second.load_state_dict(sd)
    second.load_ema_state_dict(esd)
    second.load_optimizer_state_dict(osd)
    second.refresh_shadows(all_layers=True)
    for s in (2, 3):
        second.flat_g.copy_(grads[s])
        second.step(RATES[0], **kw)
    for a, b in zip(state(straight) + [straight._ema, straight._lamb_state.trust], state(second) + [second._ema, second._lamb_state.trust]):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert straight.trust_ratios() == second.trust_ratios() and straight.step_count == second.step_count == 4


def test_stage1_one_chunk_table_one_step():
    """Stage1Engine.step(lamb=True) at the data-parallel worker's small shape: title and body engines share the flat buffers, so
    there is ONE chunk table (the title engine's); one step on the gradient of a real backward against float64."""
    import hashinit
    import synth
    from stage1 import Stage1Engine
    nl, T_, n_docs, K, Lt, Lb, B = 2, 2, 500, 3, 24, 64, 2
    eng = Stage1Engine(n_layers=nl, trainable_layers=(0, 1), num_teachers=T_, npratio=K, title_len=Lt, body_len=Lb, device=DEV,
                       batch=B, dtype="fp16")
    eng.load_state_dict({k: hashinit.init_tensor(11, k, tuple(shp)) for k, shp in eng.shapes.items()})
    eng.title.refresh_shadows(all_layers=True)
    eng.body.refresh_rel()
    d = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    titles, bodies = d(synth.news_table(11, n_docs, Lt)), d(synth.news_table(12, n_docs, Lb))
    tt, tb = d(synth.teacher_tables(11, T_, n_docs, 256)), d(synth.teacher_tables(12, T_, n_docs, 256))
    idx = d(np.random.RandomState(13).randint(1, n_docs, (B, K + 1)).astype(np.int32))
    eng.forward_indexed(titles, bodies, idx, torch.zeros(B, dtype=torch.int64, device=DEV), tt, tb)
    eng.backward()
    t = eng.title
    assert t.flat_g.data_ptr() == eng.body.flat_g.data_ptr() and t._lamb_state is None and eng.trust_ratios() is None
    gh = t.flat_g.cpu().numpy()
    assert np.isfinite(gh).all() and np.abs(gh).max() > 0
    pre = snapshot(t, False)
    eng.step(2e-2, lr_bert=1e-2, lamb=True, weight_decay=WD)
    want = expected(t, pre, gh, 1, 1.0, False, rates=(2e-2, 1e-2, 2e-2), gs=1.0)     # stage 1: lr_bert below the pooling head, lr above
    compare("stage 1 lamb", t, want, False)
    assert eng.trust_ratios() == t.trust_ratios()
    assert eng.body._lamb_state is None and eng.body._lamb_buffers() is t._lamb_state
    L.check_chunks(L.slots(t.slot), t.n_train, t._lamb_state.chunks_host.numpy(), t._lamb_state.tensors_host.numpy(), t._lamb_state.names)
    t.scaler.drain(t)
    assert t.scaler.skipped == 0 and t.step_count == 1


def test_two_ranks_hold_identical_bits(tmp_path):
    """Two processes over gloo on one GPU (tests/workers/lamb_rank.py): after three LAMB steps with clipping, decay and the average,
    parameters, moments, the average, a 16-bit weight copy and the trust ratios are identical on both ranks."""
    worker = os.path.join(ROOT, "tests", "workers", "lamb_rank.py")
    out = str(tmp_path / "rank%d.json")
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE="2", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT="29631")
        procs.append(subprocess.Popen([sys.executable, worker, out, "fp16", "4", "3"], env=env, stdout=subprocess.PIPE,
                                      stderr=subprocess.STDOUT, text=True))
    logs = [p.communicate(timeout=900)[0] for p in procs]
    for p, lg in zip(procs, logs):
        assert p.returncode == 0, lg[-3000:]
    a, b = (json.load(open(out % r)) for r in range(2))
    assert a == b and a["moved"] and a["steps"] + a["skipped"] == 3 and len(a["trust"]) > 10
    assert all(np.isfinite(v).all() for v in a["trust"].values())


def test_run_py_logs_the_trust_ratios_only_when_on(tmp_path):
    env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, "tiny-newsrec_amd"))
    base = [sys.executable, "-u", os.path.join(ROOT, "tiny-newsrec_amd", "run.py"), "--mode", "train", "--synthetic", "True",
            "--enable_hvd", "False", "--batch_size", "4", "--epochs", "1", "--max_steps_per_epoch", "6", "--log_steps", "2",
            "--num_words_title", "30", "--news_dim", "256", "--num_student_layers", "2", "--bert_trainable_layer", "0", "1",
            "--num_teachers", "2", "--user_log_mask", "False", "--coef", "0.2", "--model", "NAML", "--model_type", "tnlrv3",
            "--save_optimizer", "True"]
    for flag in (["--optimizer", "lamb", "--weight_decay", "0.01"], []):
        mdir = tmp_path / ("on" if flag else "off")
        r = subprocess.run(base + flag + ["--model_dir", str(mdir)], env=env, capture_output=True, text=True, timeout=600,
                           cwd=os.path.join(ROOT, "tiny-newsrec_amd"))
        out = r.stdout + r.stderr
        assert r.returncode == 0, out[-4000:]
        losses = [float(x) for x in re.findall(r"train_loss: ([-+0-9.eE]+|nan|inf)", out)]
        assert len(losses) >= 3 and all(np.isfinite(losses)), losses
        found = re.findall(r"trust ratio min ([-+0-9.eE]+|nan|inf) / median ([-+0-9.eE]+|nan|inf) / max ([-+0-9.eE]+|nan|inf) over (\d+) tensors", out)
        ck = torch.load(str(mdir / "epoch-1.pt"), map_location="cpu", weights_only=False)
        if flag:
            assert ck["train_state"]["flags"]["optimizer"] == "lamb"
        else:
            assert "optimizer" not in ck["train_state"]["flags"]                 # an adam run records the flags it always did
        if flag:
            assert len(found) == len(losses), out[-4000:]
            for lo, med, hi, cnt in found:
                assert 0.0 < float(lo) <= float(med) <= float(hi) < float("inf") and int(cnt) > 10
        else:
            assert not found and "trust ratio" not in out
