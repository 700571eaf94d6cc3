"""Global-norm gradient clipping through the engine: Engine.step(max_grad_norm=...), Stage1Engine, run.py --max_grad_norm.

As in tests/test_dp_gpu.py the gradients are random values written into eng.flat_g (no forward needed), on the 2-layer, 2-teacher
engine with hashinit weights.  The reference is tests/heads_ref.adam_step driven by tests/clip_ref.clip, in float64; the bounds are
those of tests/test_grad_clip_kernels_gpu.py (norm: the kernel's sum-of-squares bound, halved by the square root, plus the
rounding of the fp32 result; p rtol 1e-5 atol 1e-6; m, v, vmax rtol 1e-5 with a floor of 1e-5 of the buffer's largest magnitude)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import clip_ref as C                                    # noqa: E402
import heads_ref as R                                   # noqa: E402
import tnr_hip as T                                     # noqa: E402
from test_heads_kernels_gpu import check, check_abs     # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
RATES = (1e-4, 2e-5, 3e-5)                              # lr, lr_bert, lr_news_head: three learning-rate ranges
_P = {}


def make(dtype):
    import engine as E
    import hashinit
    from schema import FULL, state_shapes
    cfg = E.EngineConfig(n_layers=2, trainable_layers=(0, 1), num_teachers=2)
    if "P" not in _P:
        _P["P"] = hashinit.init_state_dict(3, state_shapes(FULL, 2, cfg.D, 2))
    eng = E.Engine(cfg, DEV, max_batch=2, dtype=dtype)
    eng.load_state_dict(_P["P"])
    return eng


def fill(eng, gen, scale):
    """Random gradient; what lies between the buckets (alignment gaps) holds zeros, as after a backward."""
    eng.flat_g.copy_(torch.randn(eng.n_train, device=DEV, generator=gen) * scale)
    pos = 0
    for s_, e_ in sorted(eng.bucket_ranges()) + [(eng.n_train, eng.n_train)]:
        if s_ > pos:
            eng.flat_g[pos:s_].zero_()
        pos = max(pos, e_)


def gen():
    return torch.Generator(device=DEV).manual_seed(5)


def state(eng):
    torch.cuda.synchronize()
    return [x.clone() for x in (eng.flat[True], eng.adam_m, eng.adam_v, eng.adam_vmax, eng.sh[1]["w1"])]


def norm64(eng):
    return float(np.sqrt((eng.flat_g.cpu().numpy().astype(np.float64) ** 2).sum()))


def norm_rtol(eng):
    """The kernels' bound of the sum of squares over the engine's slices, halved by the square root, + the fp32 result's rounding."""
    return 0.5 * C.sumsq_rtol([e_ - s_ for s_, e_ in eng.bucket_ranges()]) + 2.0 ** -24


class FakeSync:
    """A GradSync whose collectives are already complete: Engine.step(sync=...) takes the bucket-by-bucket path."""

    def __init__(self, ranges):
        self.ranges, self.pending, self.waited, self.scale = list(ranges), {b: None for b in range(len(ranges))}, [], 0.5

    def wait_bucket(self, b):
        self.pending.pop(b, None)
        self.waited.append(b)

    def wait(self):
        for b in list(self.pending):
            self.wait_bucket(b)


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_off_is_the_unclipped_step(monkeypatch, dtype):
    """step(lr), step(lr, max_grad_norm=None) and step(lr, max_grad_norm=0.0): equal bits in the parameters, the three state buffers
    and a 16-bit weight copy, the same C-ABI calls in the same order, and no clipping buffer."""
    calls = []
    real = T.call

    def recorder(name, *a):
        calls.append(name)
        return real(name, *a)
    monkeypatch.setattr(T, "call", recorder)
    outs, seqs = [], []
    for kw in ({}, {"max_grad_norm": None}, {"max_grad_norm": 0.0}):
        eng = make(dtype)
        g = gen()
        del calls[:]
        for step in range(2):
            fill(eng, g, 1e-3)
            eng.step(RATES[0], grad_scale=0.5, lr_bert=RATES[1], lr_news_head=RATES[2], **kw)
        outs.append(state(eng))
        seqs.append(list(calls))
        assert eng._clip_state is None and eng.grad_norm() is None
    assert seqs[0] == seqs[1] == seqs[2] and any(n.startswith("tnr_amsgrad_step") for n in seqs[0])
    assert not any("sumsq" in n or "clip" in n for n in seqs[0])
    for other in outs[1:]:
        assert all(torch.equal(a, b) for a, b in zip(outs[0], other))


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_threshold_above_the_norm_changes_nothing(dtype):
    """max_grad_norm = twice the float64 norm: the coefficient is exactly 1, three steps are bit-identical to the unclipped engine,
    and grad_norm() reports grad_scale * |g| within the kernels' bound."""
    outs = []
    for clipped in (False, True):
        eng = make(dtype)
        g = gen()
        for step in range(3):
            fill(eng, g, 1e-3)
            if clipped:
                want = 0.5 * norm64(eng)
                eng.step(RATES[0], grad_scale=0.5, lr_bert=RATES[1], max_grad_norm=2.0 * want)
                total, coef = eng.grad_norm()
                rtol = norm_rtol(eng)
                print("[grad-clip] %s step %d: grad_norm %.9g, float64 %.9g, err / bound %.4f" % (dtype, step, total, want, abs(total - want) / (rtol * want)))
                assert coef == 1.0 and abs(total - want) <= rtol * want
            else:
                eng.step(RATES[0], grad_scale=0.5, lr_bert=RATES[1])
        outs.append(state(eng))
        if dtype == "fp16":
            eng.scaler.drain(eng)
            assert eng.scaler.skipped == 0
    assert all(torch.equal(a, b) for a, b in zip(*outs))


@pytest.mark.parametrize("dtype,ams", [("fp16", True), ("bf16", False)])
def test_clipped_steps_against_float64(dtype, ams):
    """Gradients of magnitude 1e-3, 1e-1, 1e-4 and a threshold that clips the first two only; three learning rates, ONE coefficient
    across their ranges; grad_scale 0.5; AMSGrad behind fp16's guard and plain Adam under bf16.  Every step's norm, coefficient,
    parameters and state against heads_ref.adam_step on clip_ref's coefficient."""
    import engine as E
    scales, gs = (1e-3, 1e-1, 1e-4), 0.5
    eng = make(dtype)
    n = eng.n_train
    max_norm = 0.6 * gs * 1e-3 * float(np.sqrt(n))                  # 0.6 of the first step's expected norm
    head0 = eng.off(E.PFX + "attn.att_fc1.weight")
    e = eng.off(E.PFX + "dense.bias") + eng.slot[E.PFX + "dense.bias"][2]
    rest0 = min((e + 63) // 64 * 64, n)
    assert 0 < head0 < rest0 < n
    lr = np.full(n, RATES[0])
    lr[:head0], lr[head0:rest0] = RATES[1], RATES[2]
    ref = [eng.flat[True].cpu().numpy().astype(np.float64), np.zeros(n), np.zeros(n), np.zeros(n) if ams else None]
    g, rtol, coefs = gen(), norm_rtol(eng), []
    for s, sc in enumerate(scales):
        fill(eng, g, sc)
        gh = eng.flat_g.cpu().numpy()
        eng.step(RATES[0], grad_scale=gs, lr_bert=RATES[1], lr_news_head=RATES[2], amsgrad=ams, max_grad_norm=max_norm)
        total, coef = eng.grad_norm()
        want_total, want_coef = C.clip([gh], max_norm, gs)
        coefs.append(want_coef)
        print("[grad-clip] %s ams%d step %d: norm %.9g (float64 %.9g, err / bound %.4f), coef %.9g (float64 %.9g)" % (
            dtype, ams, s + 1, total, want_total, abs(total - want_total) / (rtol * want_total), coef, want_coef))
        assert abs(total - want_total) <= rtol * want_total and abs(coef - want_coef) <= 1e-6 * want_coef
        ref = list(R.adam_step(ref[0], gh, ref[1], ref[2], ref[3], s + 1, lr, grad_scale=gs * want_coef))
        got = [eng.flat[True], eng.adam_m, eng.adam_v] + ([eng.adam_vmax] if ams else [])
        for name, a, b in zip("pmvx", got, [r for r in ref if r is not None]):
            what = "engine clipped/%s %s ams%d step%d" % (name, dtype, ams, s + 1)
            if name == "p":
                check_abs(what, a.cpu().numpy(), b, 1e-5, 1e-6)
            else:
                check(what, a.cpu().numpy(), b, 1e-5, 1e-5)
    assert coefs[0] < 1.0 and coefs[1] < 0.01 and coefs[2] == 1.0
    if not ams:
        assert float(eng.adam_vmax.abs().max()) == 0.0
    if dtype == "fp16":
        eng.scaler.drain(eng)
        assert eng.scaler.skipped == 0 and eng.step_count == 3


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_bucketed_equals_whole(dtype):
    """With a sync whose collectives are in flight every bucket is scanned behind its own wait_bucket, in completion order, each
    once; the step is bit-identical to the one without sync, coefficient included.  fp16: an inf in the bucket that lands last
    leaves every slice untouched and counts one skipped step, and the bookkeeping afterwards is that of the never-clipped engine."""
    outs, norms, books = [], [], []
    for mode in ("whole", "bucketed", "unclipped"):
        eng = make(dtype)
        g = gen()
        ranges = eng.bucket_ranges()
        max_norm = 0.6 * 0.5 * 1e-3 * float(np.sqrt(eng.n_train))
        kw = {} if mode == "unclipped" else {"max_grad_norm": max_norm}
        for step in range(4):
            fill(eng, g, 1e-3)
            bad = dtype == "fp16" and step == 1
            if bad:
                eng.flat_g[ranges[-1][1] - 1] = float("inf")         # the last element of the bucket that lands last
            before = state(eng)[:4]
            sync = FakeSync(ranges) if mode == "bucketed" else None
            eng.step(1e-4, grad_scale=0.5, lr_bert=2e-5, sync=sync, **kw)
            if sync is not None:
                assert sync.waited == list(range(len(ranges))) and not sync.pending       # completion order, each once
            same = all(torch.equal(a, b) for a, b in zip(before, state(eng)[:4]))
            assert same == bad, (mode, step)
            if mode != "unclipped" and not bad:
                norms.append((mode, step, eng.grad_norm()))
        if dtype == "fp16":
            eng.scaler.drain(eng)
            books.append((eng.scaler.skipped, eng.step_count, int(eng.scaler.guard[1])))
        outs.append(state(eng))
    assert all(torch.equal(a, b) for a, b in zip(outs[0], outs[1]))
    assert [n[2] for n in norms if n[0] == "whole"] == [n[2] for n in norms if n[0] == "bucketed"]
    assert all(c < 1.0 for _, _, (t, c) in norms)
    assert not torch.equal(outs[0][1], outs[2][1])                  # ... and clipping did change the first moments
    if dtype == "fp16":
        assert books[0] == books[1] == books[2] == (1, 3, 1)


def test_stage1_one_clip_covers_title_and_body():
    """Stage1Engine.step(max_grad_norm=x) at the data-parallel worker's small shape (2 layers, 1 + 3 titles of 24, bodies of 64,
    B = 2): the title and body engines share one flat gradient, so one norm, one coefficient, one set of buffers."""
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
    assert eng.title.flat_g.data_ptr() == eng.body.flat_g.data_ptr()
    want = norm64(eng.title)
    assert np.isfinite(want) and want > 0
    before = eng.title.flat[True].clone()
    eng.step(1e-5, lr_bert=1e-6, max_grad_norm=0.5 * want)
    total, coef = eng.grad_norm()
    rtol = norm_rtol(eng.title)
    print("[grad-clip] stage 1: norm %.9g (float64 %.9g, err / bound %.4f), coef %.6g" % (total, want, abs(total - want) / (rtol * want), coef))
    assert abs(total - want) <= rtol * want and abs(coef - C.clip([eng.title.flat_g.cpu().numpy()], 0.5 * want)[1]) <= 1e-6 * coef
    assert eng.title.grad_norm() == eng.body.grad_norm() == (total, coef)
    assert eng.body._clip_owner is eng.title and eng.body._clip_state is None
    assert eng.body._clip_buffers() is eng.title._clip_state and eng.title._clip_state.part.numel() == sum(
        T.query("tnr_grad_sumsq_parts", e_ - s_) for s_, e_ in eng.bucket_ranges())
    torch.cuda.synchronize()
    assert not torch.equal(before, eng.title.flat[True]) and bool(torch.isfinite(eng.title.flat[True]).all())


def test_run_py_logs_the_gradient_norm_only_when_asked(tmp_path):
    env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, "tiny-newsrec_amd"))
    base = [sys.executable, "-u", os.path.join(ROOT, "tiny-newsrec_amd", "run.py"), "--mode", "train", "--synthetic", "True",
            "--enable_hvd", "False", "--batch_size", "4", "--epochs", "1", "--max_steps_per_epoch", "6", "--log_steps", "2",
            "--num_words_title", "30", "--news_dim", "256", "--num_student_layers", "2", "--bert_trainable_layer", "0", "1",
            "--num_teachers", "2", "--user_log_mask", "False", "--coef", "0.2", "--model", "NAML", "--model_type", "tnlrv3"]
    for flag in (["--max_grad_norm", "0.05"], []):
        r = subprocess.run(base + flag + ["--model_dir", str(tmp_path / ("on" if flag else "off"))], env=env, capture_output=True,
                           text=True, timeout=600, cwd=os.path.join(ROOT, "tiny-newsrec_amd"))
        out = r.stdout + r.stderr
        assert r.returncode == 0, out[-4000:]
        losses = [float(x) for x in re.findall(r"train_loss: ([-+0-9.eE]+|nan|inf)", out)]
        assert len(losses) >= 3 and all(np.isfinite(losses)), losses
        found = re.findall(r"grad norm ([-+0-9.eE]+|nan|inf) \(clip x([-+0-9.eE]+|nan|inf)\)", out)
        if flag:
            assert len(found) == len(losses), out[-4000:]
            assert all(np.isfinite(float(a)) and float(a) > 0 and 0 < float(b) <= 1 for a, b in found), found
        else:
            assert not found and "grad norm" not in out
