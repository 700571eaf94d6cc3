"""Gradient accumulation through the engine: Engine.backward(micro=(j, K)), the step() assertion, TnrAdam(grad_accum_steps=) and
run.py --grad_accum_steps.

The 2-layer, 2-teacher engine of tests/workers/dp_rank.py (both layers trainable, hashinit weights, synthetic news, teacher tables
and impressions), max_batch 2.  The window's sum is one correctly rounded fp32 add per element and micro-batch, so everything that
compares a window with the sum of plain backwards is BIT-exact (torch's fp32 `+` is the reference); only the comparison of K
micro-batches of B / K impressions with one batch of B has bounds, and they are those of tests/test_dp_gpu.py, which makes
numerically the same comparison (the fp32 sum of two half-batch gradients against the whole batch's)."""
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import tnr_hip as T                                     # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
NL, NT, N_NEWS, SEED = 2, 2, 3000, 7
_C = {}


def cfg():
    import engine as E
    return E.EngineConfig(n_layers=NL, trainable_layers=(0, 1), num_teachers=NT)


def weights():
    if "P" not in _C:
        import hashinit
        from schema import FULL, state_shapes
        _C["P"] = hashinit.init_state_dict(SEED, state_shapes(FULL, NL, cfg().D, NT))
    return _C["P"]


def make(dtype, max_batch=2):
    import engine as E
    eng = E.Engine(cfg(), DEV, max_batch=max_batch, dtype=dtype)
    eng.load_state_dict(weights())
    return eng


def data():
    """news table, teacher tables and 12 impressions; shared, never modified"""
    if "D" not in _C:
        import synth
        c = cfg()
        d = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
        _C["D"] = (d(synth.news_table(SEED, N_NEWS, c.L)), d(synth.teacher_tables(SEED, NT, N_NEWS, c.D)),
                   [d(x) for x in synth.impressions(SEED + 1, 12, N_NEWS, c.U, c.C)])
    return _C["D"]


def fwd(eng, first, n=2):
    comb, tabs, (hidx, mask, cidx, label) = data()
    s = slice(first, first + n)
    eng.forward_indexed(comb, hidx[s], mask[s], cidx[s], label[s], tabs)


def state(eng):
    torch.cuda.synchronize()
    return [x.clone() for x in (eng.flat[True], eng.adam_m, eng.adam_v, eng.adam_vmax, eng.sh[1]["w1"])]


def same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def plain(dtype):
    """The three plain backwards (impressions 0-1, 2-3, 4-5) of one engine, each flat_g cloned; the third once more with a no-op
    bucket hook; and their fp32 sums in the window's order.  Computed once per dtype, never modified."""
    if ("plain", dtype) not in _C:
        eng = make(dtype)
        g = []
        for j in range(3):
            fwd(eng, 2 * j)
            eng.backward()
            g.append(eng.flat_g.clone())
        fwd(eng, 4)
        eng.backward(after_bucket=lambda b: None)
        gh = eng.flat_g.clone()
        torch.cuda.synchronize()
        _C["plain", dtype] = types.SimpleNamespace(g=g, g_last_hooked=gh, total=(g[0] + g[1]) + g[2], total_hooked=(g[0] + g[1]) + gh)
    return _C["plain", dtype]


def record(monkeypatch):
    calls = []
    real = T.call

    def recorder(name, *a):
        calls.append(name)
        return real(name, *a)
    monkeypatch.setattr(T, "call", recorder)
    return calls


def _model(dtype):
    import model_bert
    c = cfg()
    args = types.SimpleNamespace(
        config_name=None, pooling="att", model="NAML", num_teacher_layers=12, num_student_layers=NL, bert_trainable_layer=[0, 1],
        news_dim=c.D, news_query_vector_dim=c.Qn, user_query_vector_dim=c.Qu, num_teachers=NT, user_log_length=c.U,
        npratio=c.C - 1, num_words_title=c.L, user_log_mask=c.user_log_mask, temperature=c.temperature, coef=c.coef, batch_size=2,
        dtype=dtype)
    model = model_bert.Model(args, device=DEV)
    model.engine.load_state_dict(weights())
    return model


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_off_is_the_step_as_it_was(monkeypatch, dtype):
    """backward(), backward(micro=None), backward(micro=(0, 1)) and the module surface with TnrAdam(grad_accum_steps=1): the same
    C-ABI calls in the same order without tnr_grad_accum among them, no accumulator, the same bits in parameters and state."""
    import model_bert
    calls = record(monkeypatch)
    outs, seqs = [], []
    for kw in ({}, dict(micro=None), dict(micro=(0, 1)), "module"):
        if kw == "module":
            model = _model(dtype)
            eng = model.engine
            opt = model_bert.TnrAdam(model, 1e-4, grad_accum_steps=1)
        else:
            eng = make(dtype)
        del calls[:]
        for u in range(2):
            if kw == "module":
                comb, tabs, (hidx, mask, cidx, label) = data()
                s = slice(2 * u, 2 * u + 2)
                total = model.forward_indexed(comb, hidx[s], mask[s], cidx[s], label[s], tabs)[0]
                opt.zero_grad()
                total.backward()
                opt.step()
                assert model._micro is None
            else:
                fwd(eng, 2 * u)
                eng.backward(**kw)
                eng.step(1e-4)
        outs.append(state(eng))
        seqs.append(list(calls))
        assert eng._acc is None and eng._acc_held == 0
    assert all(s == seqs[0] for s in seqs[1:]) and any(n.startswith("tnr_amsgrad_step") for n in seqs[0])
    assert "tnr_grad_accum" not in seqs[0]
    for other in outs[1:]:
        assert all(same_bits(a, b) for a, b in zip(outs[0], other))


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_window_sum_is_bit_exact_and_the_step_sees_the_sum(monkeypatch, dtype):
    """K = 3: flat_g after the window is (g0 + g1) + g2 of three plain backwards, bit for bit, with one tnr_grad_accum per
    micro-batch; the step behind it (mean by grad_scale = 1 / 3, clipping, decay, average) leaves the bits of a step on a flat_g
    filled with that sum."""
    ref = plain(dtype)
    calls = record(monkeypatch)
    eng = make(dtype)
    per_micro = []
    for j in range(3):
        del calls[:]
        fwd(eng, 2 * j)
        eng.backward(micro=(j, 3))
        per_micro.append(calls.count("tnr_grad_accum"))
        assert eng._acc_held == (j + 1) % 3
    torch.cuda.synchronize()
    assert per_micro == [1, 1, 1]
    assert eng._acc is not None and eng._acc.shape == eng.flat_g.shape and eng._acc.dtype == torch.float32
    assert same_bits(eng.flat_g, ref.total)
    assert not same_bits(eng.flat_g, ref.g[2])                         # the window is not its last micro-batch alone
    _C["window", dtype] = eng.flat_g.clone()
    other = make(dtype)
    other.flat_g.copy_(ref.total)
    max_norm = 0.5 * float(ref.total.double().norm()) / 3.0            # half the mean gradient's norm: the step clips
    kw = dict(grad_scale=1.0 / 3.0, max_grad_norm=max_norm, weight_decay=0.01, ema_decay=0.9)
    eng.step(1e-4, **kw)
    other.step(1e-4, **kw)
    assert eng.grad_norm()[1] < 0.75 and eng.grad_norm() == other.grad_norm()
    for a, b in zip(state(eng) + [eng._ema], state(other) + [other._ema]):
        assert same_bits(a, b)
    assert not same_bits(eng.flat[True], make(dtype).flat[True])       # and it did update


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_with_a_hook_every_bucket_carries_the_sum_when_its_hook_fires(dtype):
    ref = plain(dtype)
    eng = make(dtype)
    ranges = eng.bucket_ranges()
    fired, clones = [], []

    def hook(b):
        fired.append(b)
        s_, e_ = ranges[b]
        clones.append(eng.flat_g[s_:e_].clone())
    for j in range(3):
        fwd(eng, 2 * j)
        eng.backward(after_bucket=hook, micro=(j, 3))
        if j < 2:
            assert fired == []                                         # no collective would have started
    torch.cuda.synchronize()
    assert fired == list(range(len(ranges))) and eng._acc_held == 0
    for b, (s_, e_) in enumerate(ranges):
        assert same_bits(clones[b], ref.total_hooked[s_:e_]), "bucket %d did not hold the window's sum when its hook fired" % b
    if ("window", dtype) not in _C:                                    # the no-hook window (the test above leaves it here)
        other = make(dtype)
        for j in range(3):
            fwd(other, 2 * j)
            other.backward(micro=(j, 3))
        _C["window", dtype] = other.flat_g.clone()
    for s_, e_ in ranges:
        assert same_bits(eng.flat_g[s_:e_], _C["window", dtype][s_:e_])


def test_fp16_overflow_in_any_micro_batch_skips_the_whole_update_as_one():
    eng = make("fp16")
    fwd(eng, 0)
    eng.backward(micro=(0, 2))
    eng._acc[eng.n_train // 2] = float("inf")                          # as if micro-batch 0's backward had overflowed
    fwd(eng, 2)
    eng.backward(micro=(1, 2))
    before = state(eng)[:4]
    assert not bool(torch.isfinite(eng.flat_g).all())
    eng.step(1e-4, grad_scale=0.5)
    assert all(same_bits(a, b) for a, b in zip(before, state(eng)[:4]))
    eng.scaler.drain(eng)
    assert eng.scaler.skipped == 1 and eng.step_count == 0
    eng._acc.fill_(float("nan"))                                       # what an abandoned window may leave behind
    fwd(eng, 4)
    eng.backward(micro=(0, 2))
    fwd(eng, 6)
    eng.backward(micro=(1, 2))
    eng.step(1e-4, grad_scale=0.5)
    eng.scaler.drain(eng)
    after = state(eng)[:4]
    assert eng.scaler.skipped == 1 and eng.step_count == 1
    assert all(bool(torch.isfinite(x).all()) for x in after) and bool(torch.isfinite(eng.flat_g).all())
    assert not same_bits(before[0], after[0])


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_two_micro_batches_of_two_equal_one_batch_of_four(dtype):
    """K = 2 windows of 2 impressions with grad_scale = 1 / 2 against one engine at 4 impressions: tests/test_dp_gpu.py's
    comparison of two ranks with one, and its bounds."""
    import engine as E
    lr, steps = 1e-4, 2
    acc, one = make(dtype), make(dtype, max_batch=4)
    for u in range(steps):
        for j in range(2):
            fwd(acc, 4 * u + 2 * j)
            acc.backward(micro=(j, 2))
        fwd(one, 4 * u, 4)
        one.backward()
        if u == 0:
            g2, g1 = (0.5 * acc.flat_g).cpu().numpy().astype(np.float64), one.flat_g.cpu().numpy().astype(np.float64)
        acc.step(lr, grad_scale=0.5)
        one.step(lr)
    cut = acc.off(E.PFX + "dense.weight")
    for name, sl in (("encoder + pooling", slice(0, cut)), ("heads", slice(cut, None))):
        rel = np.linalg.norm(g2[sl] - g1[sl]) / np.linalg.norm(g1[sl])
        print("%s %s: rel. L2 difference of the averaged gradient %.2e" % (dtype, name, rel))
        assert rel < (1e-3 if dtype == "fp16" else 8e-3), (name, rel)
    dp = np.abs(acc.flat[True].cpu().numpy().astype(np.float64) - one.flat[True].cpu().numpy().astype(np.float64))
    print("%s: |param diff| mean %.2e max %.2e (lr %.0e)" % (dtype, dp.mean(), dp.max(), lr))
    assert dp.mean() < 0.02 * lr and dp.max() <= 2.05 * lr * steps


def test_misuse_raises():
    import model_bert
    eng = make("bf16")
    fwd(eng, 0)
    with pytest.raises(AssertionError, match="holds 0 micro-gradients"):
        eng.backward(micro=(1, 3))                                     # nothing is held
    eng.backward(micro=(0, 3))
    with pytest.raises(AssertionError, match=r"step\(\) inside an accumulation window"):
        eng.step(1e-4)
    with pytest.raises(AssertionError, match="holds 1 micro-gradients"):
        eng.backward(micro=(0, 3))                                     # one is held
    before = state(eng)[0]
    eng.accum_reset()                                                  # drops the partial window
    assert eng._acc_held == 0
    fwd(eng, 2)
    eng.backward(micro=(0, 3))
    eng.accum_reset()
    fwd(eng, 4)
    eng.backward()
    eng.step(1e-4)
    assert not same_bits(before, state(eng)[0])
    stub = types.SimpleNamespace(strict_grad_scale=True, engine=eng, _micro=None)
    with pytest.raises(ValueError, match="strict_grad_scale"):
        model_bert.TnrAdam(stub, 1e-4, grad_accum_steps=2)


@pytest.mark.parametrize("flag", [["--grad_accum_steps", "2", "--max_grad_norm", "0.05"], ["--grad_accum_steps", "4"], []],
                         ids=["K2_clipped", "K4", "off"])
def test_run_py_with_and_without_the_flag(tmp_path, flag):
    env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, "tiny-newsrec_amd"))
    base = [sys.executable, "-u", os.path.join(ROOT, "tiny-newsrec_amd", "run.py"), "--mode", "train", "--synthetic", "True",
            "--enable_hvd", "False", "--batch_size", "4", "--epochs", "1", "--max_steps_per_epoch", "6", "--log_steps", "2",
            "--num_words_title", "30", "--news_dim", "256", "--num_student_layers", "2", "--bert_trainable_layer", "0", "1",
            "--num_teachers", "2", "--user_log_mask", "False", "--coef", "0.2", "--model", "NAML", "--model_type", "tnlrv3"]
    mdir = tmp_path / "model"
    r = subprocess.run(base + flag + ["--model_dir", str(mdir)], env=env, capture_output=True, text=True, timeout=600,
                       cwd=os.path.join(ROOT, "tiny-newsrec_amd"))
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    losses = [float(x) for x in re.findall(r"train_loss: ([-+0-9.eE]+|nan|inf)", out)]
    assert len(losses) >= 3 and all(np.isfinite(losses)), losses
    ck = torch.load(os.path.join(str(mdir), "epoch-1.pt"), map_location="cpu")
    assert set(ck) == {"model_state_dict", "category_dict", "word_dict", "subcategory_dict"}
    assert all(bool(torch.isfinite(v).all()) for v in ck["model_state_dict"].values())
    left = re.findall(r"--grad_accum_steps (\d+): the last (\d+) batch", out)
    norms = re.findall(r"grad norm ([-+0-9.eE]+|nan|inf) \(clip x([-+0-9.eE]+|nan|inf)\)", out)
    if flag and flag[1] == "2":
        assert not left, out[-4000:]                               # 6 batches: three full windows
        assert norms and all(np.isfinite(float(a)) and float(a) > 0 and 0 < float(b) <= 1 for a, b in norms), norms
    elif flag:
        assert left == [("4", "2")] and not norms, out[-4000:]     # one window and two batches left over, said once
    else:
        assert not left and not norms and "fall outside a full window" not in out
