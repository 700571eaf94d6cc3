"""Decoupled weight decay and the warmup / decay schedule through the engine: Engine.step(weight_decay=, warmup_steps=,
lr_decay_steps=), Stage1Engine, run.py --weight_decay / --warmup_steps / --lr_decay_steps.

The 2-layer, 2-teacher hashinit engine and the random-flat_g pattern of tests/test_grad_clip_gpu.py (its helpers are imported).
The reference is tests/adamw_ref.adamw_step in float64 with the mask of adamw_ref.decay_mask on the engine's own slot table; the
bounds are the optimiser tests' own (p rtol 1e-5 atol 1e-6; m, v, vmax rtol 1e-5 with a floor of 1e-5 of the buffer's largest
magnitude).  weight_decay is 0.01, the usual fine-tuning value; the learning rates are large on purpose (2e-2, 1e-2, 5e-3)
so that the decay, lr x wd = 5e-5 ... 2e-4 per full-rate step, stands well above the parameter bound: each case also asserts that
the float64 reference WITHOUT decay misses the engine's parameters by more than that bound."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import adamw_ref as A                                   # noqa: E402
import clip_ref as C                                    # noqa: E402
import tnr_hip as T                                     # noqa: E402
from test_heads_kernels_gpu import check, check_abs     # noqa: E402
from test_grad_clip_gpu import make, fill, gen, state, FakeSync, ROOT, DEV     # noqa: E402

RATES = (2e-2, 1e-2, 5e-3)                              # lr, lr_bert, lr_news_head
WD, W, TD, GS = 0.01, 2, 5, 0.5
ON = dict(weight_decay=WD, warmup_steps=W, lr_decay_steps=TD)


def tables(eng, rates=RATES):
    """Per-element learning rate (the three ranges of Engine.step) and decay mask (adamw_ref.decay_mask on the slot table)."""
    import engine as E
    n = eng.n_train
    head0 = eng.off(E.PFX + "attn.att_fc1.weight")
    e = eng.off(E.PFX + "dense.bias") + eng.slot[E.PFX + "dense.bias"][2]
    rest0 = min((e + 63) // 64 * 64, n)
    assert 0 < head0 < rest0 <= n
    lr = np.full(n, rates[0])
    lr[:head0], lr[head0:rest0] = rates[1], rates[2]
    tr = [(k, v) for k, v in eng.slot.items() if v[0]]
    mask = A.decay_mask([k for k, _ in tr], [v[3] for _, v in tr], [v[1] for _, v in tr], n)
    assert 0 < mask.sum() < n and mask[:head0].any() and mask[head0:rest0].any() and (rest0 == n or mask[rest0:].any())
    return lr, mask


def ref_state(eng, ams):
    n = eng.n_train
    return [eng.flat[True].cpu().numpy().astype(np.float64), np.zeros(n), np.zeros(n), np.zeros(n) if ams else None]


def compare(what, eng, ref, ams):
    got = [eng.flat[True], eng.adam_m, eng.adam_v] + ([eng.adam_vmax] if ams else [])
    for name, a, b in zip("pmvx", got, [r for r in ref if r is not None]):
        if name == "p":
            check_abs("%s/p" % what, a.cpu().numpy(), b, 1e-5, 1e-6)
        else:
            check("%s/%s" % (what, name), a.cpu().numpy(), b, 1e-5, 1e-5)


def decay_shows(eng, ref_nodecay, mask):
    """The same float64 run without decay misses the engine's parameters by more than the bound, in decayed elements only."""
    got = eng.flat[True].cpu().numpy().astype(np.float64)
    over = np.abs(got - ref_nodecay) > 1e-6 + 1e-5 * np.abs(ref_nodecay)
    assert over[mask].any() and not over[~mask].any()


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_off_is_the_step_as_it_was(monkeypatch, dtype):
    """Absent / None / 0: the same C-ABI calls in the same order, the same bits in parameters, state and one 16-bit weight copy, no
    map, no multiplier."""
    calls = []
    real = T.call

    def recorder(name, *a):
        calls.append(name)
        return real(name, *a)
    monkeypatch.setattr(T, "call", recorder)
    outs, seqs = [], []
    for kw in ({}, dict(weight_decay=None, warmup_steps=None, lr_decay_steps=None), dict(weight_decay=0.0, warmup_steps=0, lr_decay_steps=0)):
        eng = make(dtype)
        g = gen()
        del calls[:]
        for step in range(2):
            fill(eng, g, 1e-3)
            eng.step(RATES[0], grad_scale=GS, lr_bert=RATES[1], lr_news_head=RATES[2], **kw)
        outs.append(state(eng))
        seqs.append(list(calls))
        assert eng._decay_map is None and eng.lr_scale is None
    assert seqs[0] == seqs[1] == seqs[2] and any(n.startswith("tnr_amsgrad_step") for n in seqs[0])
    assert "tnr_adamw_step" not in seqs[0]
    for other in outs[1:]:
        assert all(torch.equal(a, b) for a, b in zip(outs[0], other))
    # ... and any of the three alone sends every launch through the new entry point
    for kw in (dict(weight_decay=WD), dict(warmup_steps=1), dict(lr_decay_steps=3)):
        eng = make(dtype)
        fill(eng, gen(), 1e-3)
        del calls[:]
        eng.step(RATES[0], grad_scale=GS, lr_bert=RATES[1], lr_news_head=RATES[2], **kw)
        assert calls.count("tnr_adamw_step") == 3 and not any(n.startswith("tnr_amsgrad_step") for n in calls), (kw, calls)
        assert (eng._decay_map is not None) == ("weight_decay" in kw) and (eng.lr_scale is None) == ("weight_decay" in kw)


@pytest.mark.parametrize("clipped", [False, True])
@pytest.mark.parametrize("dtype,ams", [("fp16", True), ("bf16", False)])
def test_three_steps_against_float64(dtype, ams, clipped):
    """Three learning-rate ranges, wd = 0.01, W = 2, T = 5 (multipliers 0, 1/2, 1), grad_scale 0.5; AMSGrad behind fp16's guard and
    plain Adam under bf16, with and without max_grad_norm (which clips the first step)."""
    eng = make(dtype)
    lr, mask = tables(eng)
    max_norm = 0.6 * GS * 1e-3 * float(np.sqrt(eng.n_train))
    kw = dict(ON, max_grad_norm=max_norm) if clipped else ON
    ref, plain = ref_state(eng, ams), ref_state(eng, ams)
    p0 = eng.flat[True].clone()
    g, coefs = gen(), []
    for s, sc in enumerate((1e-3, 1e-4, 1e-3)):
        fill(eng, g, sc)
        gh = eng.flat_g.cpu().numpy()
        eng.step(RATES[0], grad_scale=GS, lr_bert=RATES[1], lr_news_head=RATES[2], amsgrad=ams, **kw)
        mult = A.schedule(s, W, TD)
        assert eng.lr_scale == mult == (0.0, 0.5, 1.0)[s]
        coef = C.clip([gh], max_norm, GS)[1] if clipped else 1.0
        coefs.append(coef)
        ref = list(A.adamw_step(ref[0], gh, ref[1], ref[2], ref[3], s + 1, lr * mult, mask, WD, grad_scale=GS * coef))
        plain = list(A.adamw_step(plain[0], gh, plain[1], plain[2], plain[3], s + 1, lr * mult, False, WD, grad_scale=GS * coef))
        compare("engine adamw %s ams%d clip%d step%d" % (dtype, ams, clipped, s + 1), eng, ref, ams)
        if s == 0:
            assert torch.equal(eng.flat[True], p0)                           # the first update of a warmup has rate 0
    assert (coefs[0] < 1.0 and coefs[1] == 1.0) if clipped else coefs == [1.0] * 3
    decay_shows(eng, plain[0], mask)
    words = A.unpack(eng._decay_map.cpu().numpy(), eng.n_train)
    assert (words == mask).all()
    if not ams:
        assert float(eng.adam_vmax.abs().max()) == 0.0
    if dtype == "fp16":
        eng.scaler.drain(eng)
        assert eng.scaler.skipped == 0 and eng.step_count == 3


@pytest.mark.parametrize("clipped", [False, True])
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_bucketed_equals_whole(dtype, clipped):
    """A sync whose collectives are complete but pending sends bf16 through the bucket-by-bucket update (`first` at the bucket x
    range boundaries) and fp16 through the per-bucket scans: bit-identical to the step without sync."""
    outs = []
    for mode in ("whole", "bucketed"):
        eng = make(dtype)
        p0 = eng.flat[True].clone()
        g = gen()
        ranges = eng.bucket_ranges()
        kw = dict(ON, max_grad_norm=0.6 * GS * 1e-3 * float(np.sqrt(eng.n_train))) if clipped else ON
        for step in range(3):
            fill(eng, g, 1e-3)
            sync = FakeSync(ranges) if mode == "bucketed" else None
            eng.step(RATES[0], grad_scale=GS, lr_bert=RATES[1], lr_news_head=RATES[2], amsgrad=dtype == "fp16", sync=sync, **kw)
            if sync is not None:
                assert sync.waited == list(range(len(ranges))) and not sync.pending
        outs.append(state(eng))
        if dtype == "fp16":
            eng.scaler.drain(eng)
            assert eng.scaler.skipped == 0
    assert all(torch.equal(a, b) for a, b in zip(*outs))
    assert not torch.equal(outs[0][0], p0)


def test_fp16_skipped_step_advances_neither_count_nor_schedule():
    """Six steps with W = 4 and an inf written into flat_g at the third: one skip, which decays nothing and moves nothing; the
    parameters are those of the float64 reference that takes FIVE updates with multipliers 0, 1/4, 2/4, 3/4, 1 and bias corrections
    1 ... 5 - the step behind the skip runs before the host knows of it and picks its rate on the device."""
    eng = make("fp16")
    lr, mask = tables(eng)
    ref, plain = ref_state(eng, True), ref_state(eng, True)
    g, taken, seen = gen(), 0, []
    for step in range(6):
        fill(eng, g, 1e-3)
        if step == 2:
            eng.flat_g[eng.n_train // 2 + 1] = float("inf")
        gh = eng.flat_g.cpu().numpy()
        before = state(eng)[:4]
        eng.step(RATES[0], grad_scale=GS, lr_bert=RATES[1], lr_news_head=RATES[2], weight_decay=WD, warmup_steps=4)
        seen.append(eng.lr_scale)
        if step == 2:
            assert all(torch.equal(a, b) for a, b in zip(before, state(eng)[:4]))       # nothing decayed, nothing moved
            continue
        mult = A.schedule(taken, 4, 0)
        taken += 1
        ref = list(A.adamw_step(ref[0], gh, ref[1], ref[2], ref[3], taken, lr * mult, mask, WD, grad_scale=GS))
        plain = list(A.adamw_step(plain[0], gh, plain[1], plain[2], plain[3], taken, lr * mult, False, WD, grad_scale=GS))
        compare("engine adamw skip: step %d = update %d (x%.2f)" % (step + 1, taken, mult), eng, ref, True)
    eng.scaler.drain(eng)
    assert eng.scaler.skipped == 1 and eng.step_count == 5 and int(eng.scaler.guard[1]) == 1 and taken == 5
    # the host's multiplier runs ahead of the device's by the skip it has not heard of yet (steps 3 and 4), then falls back
    assert seen == [0.0, 0.25, 0.5, 0.75, 0.75, 1.0]
    decay_shows(eng, plain[0], mask)


def test_stage1_one_map_one_schedule():
    """Stage1Engine.step with decay + schedule at the data-parallel worker's small shape: the title and body engines share the
    flat buffers, so there is one map (the title engine's) and one schedule position.  Two steps on the gradient of one backward
    (the update does not consume it): the first has rate 0, the second half the rate."""
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
    assert t.flat_g.data_ptr() == eng.body.flat_g.data_ptr() and t._decay_map is None
    gh = t.flat_g.cpu().numpy()
    assert np.isfinite(gh).all() and np.abs(gh).max() > 0
    lr, mask = tables(t, (2e-2, 1e-2, 2e-2))                   # stage 1 has two ranges: lr_bert below the pooling head, lr above
    ref, plain = ref_state(t, False), ref_state(t, False)
    for s in range(2):
        eng.step(2e-2, lr_bert=1e-2, **ON)
        mult = A.schedule(s, W, TD)
        assert eng.lr_scale == t.lr_scale == mult
        ref = list(A.adamw_step(ref[0], gh, ref[1], ref[2], None, s + 1, lr * mult, mask, WD))
        plain = list(A.adamw_step(plain[0], gh, plain[1], plain[2], None, s + 1, lr * mult, False, WD))
        compare("stage 1 adamw step%d" % (s + 1), t, ref, False)
    decay_shows(t, plain[0], mask)
    assert eng.body._decay_map is None and eng.body._decay_bits() is t._decay_map and eng.body.lr_scale is None
    assert (A.unpack(t._decay_map.cpu().numpy(), t.n_train) == mask).all()
    t.scaler.drain(t)
    assert t.scaler.skipped == 0 and t.step_count == 2


def test_run_py_logs_the_multiplier_only_when_a_schedule_is_on(tmp_path):
    env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, "tiny-newsrec_amd"))
    base = [sys.executable, "-u", os.path.join(ROOT, "tiny-newsrec_amd", "run.py"), "--mode", "train", "--synthetic", "True",
            "--enable_hvd", "False", "--batch_size", "4", "--epochs", "1", "--max_steps_per_epoch", "6", "--log_steps", "2",
            "--num_words_title", "30", "--news_dim", "256", "--num_student_layers", "2", "--bert_trainable_layer", "0", "1",
            "--num_teachers", "2", "--user_log_mask", "False", "--coef", "0.2", "--model", "NAML", "--model_type", "tnlrv3"]
    for flag in (["--weight_decay", "0.01", "--warmup_steps", "4", "--lr_decay_steps", "100"], []):
        r = subprocess.run(base + flag + ["--model_dir", str(tmp_path / ("on" if flag else "off"))], env=env, capture_output=True,
                           text=True, timeout=600, cwd=os.path.join(ROOT, "tiny-newsrec_amd"))
        out = r.stdout + r.stderr
        assert r.returncode == 0, out[-4000:]
        losses = [float(x) for x in re.findall(r"train_loss: ([-+0-9.eE]+|nan|inf)", out)]
        assert len(losses) >= 3 and all(np.isfinite(losses)), losses
        found = [float(x) for x in re.findall(r", lr x([0-9.eE+-]+)", out)]
        if flag:
            # run.py logs behind its steps 1, 3, 5 (it counts from 0): multipliers s(0), s(2), s(4) of W = 4, T = 100 when no step
            # was skipped; a skipped step (fp16 overflow) can only hold the schedule back
            assert len(found) == len(losses), out[-4000:]
            want = [A.schedule(u, 4, 100) for u in (0, 2, 4)]
            assert want == [0.0, 0.5, 1.0]
            assert all(0.0 <= a <= b + 1e-4 for a, b in zip(found, want)) and found == sorted(found), (found, want)
            if "steps skipped" not in out:
                assert np.allclose(found, want, rtol=1e-3), (found, want)
        else:
            assert not found and "lr x" not in out
