"""GPU: in-batch negatives in the target loss at engine level (Engine.forward(inbatch_ids=...), forward_indexed(inbatch=True)), both
16-bit types.

Model: history_ref's (hidden 256, two layers, U, C, L = 20, 5, 17, news_dim 64, two teachers) with the weights and variants of
tests/variants_ref.py; feeds: inbatch_ref.engine_feed - indices into the first 13 rows of history_ref's news table, so that ids
collide in every way the five rules care about (tests/test_inbatch_ref_cpu.py holds them to the fixture condition), B = 3, 4, 5.

The whole step is held to torch autograd: oracle/torch_port.py's news_encoder / user_encoder as they are, the extended loss written
below from the definition (include/tnr_hip.h), under widths_ref.TOLS (fp16: loss 2e-3, score 3e-3 of max(1, |ref|), gradients 2e-2
relative L2; bf16: 1.6e-2, 2.4e-2, 8e-2), every gradient key through variants_ref.compare_grads.  Everything else is bit equality
between two runs of the engine that must not differ."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import engine as E                                               # noqa: E402
import history_ref as HR                                         # noqa: E402
import inbatch_ref as R                                          # noqa: E402
import tnr_hip as T                                              # noqa: E402
import variants_ref as V                                         # noqa: E402
import widths_ref as W                                           # noqa: E402
from dedup import build_plan                                     # noqa: E402
from oracle import torch_port as TP                              # noqa: E402
from test_step_history_gpu import DEV, _shared, _t               # noqa: E402

NEW = ("tnr_inbatch_plan", "tnr_inbatch_loss", "tnr_inbatch_bwd")
_DEVF, _PORT = {}, {}


def dfeed(name, B=None):
    """Device tensors (hist_idx, cand_idx, mask, label) of an engine fixture (its first B impressions)."""
    if (name, B) not in _DEVF:
        _DEVF[name, B] = tuple(_t(x[:B]) for x in R.engine_feed(name))
    return _DEVF[name, B]


def weights(model, teachers):
    P = _shared(model)["P"]
    return P if teachers else {k: v for k, v in P.items() if not k.startswith(("teachers.", "transform_matrix."))}


def make(dtype, B, model="att", teachers=True, **more):
    kw = dict(V.engine_kwargs(model), num_teachers=HR.T_ if teachers else 0, **more)
    eng = E.Engine(E.EngineConfig(**kw), DEV, max_batch=B, dtype=dtype)
    eng.load_state_dict(weights(model, teachers))
    return eng


def run(eng, name, on, B=None, plan=None, form="idx", micro=None, model="att", backward=True):
    """forward + backward of one fixture -> clones of losses, score, flat_g (and the eligible counts when on)."""
    s = _shared(model)
    h, c, m, y = dfeed(name, B)
    teachers = eng.cfg.T > 0
    if form == "idx":
        kw = dict(inbatch=True) if on else ({} if on is None else dict(inbatch=False))
        losses, score = eng.forward_indexed(s["comb"], h, m, c, y, s["tables"] if teachers else None, plan=plan, **kw)
    else:
        th = [s["tables"][i][h.long()] for i in range(HR.T_)] if teachers else None
        tc = [s["tables"][i][c.long()] for i in range(HR.T_)] if teachers else None
        losses, score = eng.forward(s["comb"][h.long()].long(), m, s["comb"][c.long()].long(), y, th, tc, plan=plan,
                                    inbatch_ids=(h, c) if on else None)
    out = dict(losses=losses.clone(), score=score.clone())
    if on:
        out["count"] = eng.inbatch_counts().clone()
    if backward:
        eng.backward(micro=micro)
        out["flat_g"] = eng.flat_g.clone()
    return out


def same(a, b, keys=("losses", "score", "flat_g")):
    return [k for k in keys if not torch.equal(a[k], b[k])]


# ---------------------------------------------------------------------------------------------------------------- off
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_off_is_the_step_as_it_was(monkeypatch, dtype):
    """Absent / None / False: the same C-ABI calls in the same order, the same bits, no buffer.  On: the sequence gains
    tnr_inbatch_plan in front, tnr_inbatch_loss behind tnr_kd_score_loss and tnr_inbatch_bwd between tnr_score_bwd and
    tnr_user_bwd_pre; nothing else moves."""
    calls = []
    real = T.call

    def recorder(name, *a):
        calls.append(name)
        return real(name, *a)
    monkeypatch.setattr(T, "call", recorder)
    s = _shared("att")
    h, c, m, y = dfeed("e4")
    idx = dict(teacher_tables=s["tables"], t_hidx=h, t_cidx=c, news_combined=s["comb"])
    forms = [lambda e: e.forward_indexed(s["comb"], h, m, c, y, s["tables"]),
             lambda e: e.forward_indexed(s["comb"], h, m, c, y, s["tables"], inbatch=False),
             lambda e: e.forward(None, m, None, y, **idx),
             lambda e: e.forward(None, m, None, y, inbatch_ids=None, **idx),
             lambda e: e.forward(None, m, None, y, inbatch_ids=False, **idx)]
    outs, seqs = [], []
    for f in forms:
        eng = make(dtype, 4)
        del calls[:]
        losses, score = f(eng)
        eng.backward()
        outs.append(dict(losses=losses.clone(), score=score.clone(), flat_g=eng.flat_g.clone()))
        seqs.append(list(calls))
        assert eng._inbatch is None and not eng._ib_on
        with pytest.raises(RuntimeError):
            eng.inbatch_counts()
    assert all(q == seqs[0] for q in seqs[1:]) and not any(n in NEW for n in seqs[0])
    assert all(not same(outs[0], o) for o in outs[1:])
    assert seqs[0].count("tnr_kd_score_loss") == 1 and seqs[0].count("tnr_score_bwd") == 1
    want = [NEW[0]]
    for n in seqs[0]:
        want.append(n)
        if n == "tnr_kd_score_loss":
            want.append(NEW[1])
        if n == "tnr_score_bwd":
            want.append(NEW[2])
    assert want[want.index(NEW[2]) + 1] == "tnr_user_bwd_pre"
    eng = make(dtype, 4)
    del calls[:]
    on = run(eng, "e4", True)
    assert calls == want, [(i, a, b) for i, (a, b) in enumerate(zip(calls, want)) if a != b][:3]
    assert eng._inbatch is not None and torch.equal(on["score"], outs[0]["score"])
    assert torch.equal(on["losses"][0], outs[0]["losses"][0]) and torch.equal(on["losses"][2], outs[0]["losses"][2])
    assert not torch.equal(on["losses"][1], outs[0]["losses"][1]) and not torch.equal(on["flat_g"], outs[0]["flat_g"])


# ---------------------------------------------------------------------------------------------------------------- autograd
def _news_vectors(P, x2l, cfg):
    """torch_port.news_encoder; under mean / cls pooling with its att_pool standing aside while it runs (variants_ref.port_grads'
    way: the port's own embedding block and layers, the pooling swapped for x.mean(1) / x[:, 0])."""
    if cfg["pooling"] == "att":
        return TP.news_encoder(P, x2l, cfg["n_layers"], cfg["heads"])
    assert cfg["pooling"] in ("mean", "cls")
    captured, keep = {}, TP.att_pool
    TP.att_pool = lambda x, *w, **kw: captured.setdefault("x", x)[:, 0]
    try:
        P2 = dict(P)
        for k in ("attn.att_fc1.weight", "attn.att_fc1.bias", "attn.att_fc2.weight", "attn.att_fc2.bias"):
            P2.setdefault(TP.PFX + k, None)
        TP.news_encoder(P2, x2l, cfg["n_layers"], cfg["heads"])
    finally:
        TP.att_pool = keep
    x = captured["x"]
    return F.linear(x.mean(1) if cfg["pooling"] == "mean" else x[:, 0], P[TP.PFX + "dense.weight"], P[TP.PFX + "dense.bias"])


def port_step(model, name, teachers, embed=False):
    """Model.forward (torch_port.model_forward's formulas) with the target term over own + eligible foreign candidates, and its
    autograd gradients.  -> (losses [distill, target, emb] float64, score (B, C), {key: gradient}); computed once.
    embed: the five embedding parameters train as well (embed_train_ref.port_grads' way)."""
    key = (model, name, teachers, embed)
    if key in _PORT:
        return _PORT[key]
    cfg = V.oracle_cfg(model)
    Pn = V.weights(model)
    if not teachers:
        Pn = {k: v for k, v in Pn.items() if not k.startswith(("teachers.", "transform_matrix."))}
    P = TP.make_params(Pn, cfg["trainable_layers"])
    if embed:
        from embed_train_ref import EMB_KEYS
        for k in EMB_KEYS:
            P[k].requires_grad_(True)
    h, c, m, y = R.engine_feed(name)
    El = torch.from_numpy(R.eligibility(h, c).astype(bool))
    h, c = torch.from_numpy(h.astype(np.int64)), torch.from_numpy(c.astype(np.int64))
    B, U, C = h.shape[0], h.shape[1], c.shape[1]
    comb, tt = torch.from_numpy(HR.news().astype(np.int64)), torch.from_numpy(HR.teachers())
    mask, label = torch.from_numpy(m), torch.from_numpy(y)
    allx = torch.cat([comb[h.reshape(-1)], comb[c.reshape(-1)]], 0)
    vec = _news_vectors(P, allx, cfg)
    D = vec.shape[1]
    hist, cand = vec[:B * U].view(B, U, D), vec[B * U:].view(B, C, D)
    user = TP.user_encoder(P, "student.user_encoder.", hist, mask, cfg["user_log_mask"])
    score = torch.bmm(cand, user[:, :, None])[..., 0]
    # the extended target term
    z = user @ cand.reshape(B * C, D).T
    target = torch.stack([-torch.log_softmax(torch.cat([score[b], z[b][El[b]]]), 0)[label[b]] for b in range(B)]).mean()
    distill = emb = torch.zeros(())
    if teachers:
        S = torch.cat([hist, cand], 1)
        ts_all, tl, NE, UE = [], [], [], []
        for i in range(HR.T_):
            Wt, bt = P["transform_matrix.%d.weight" % i], P["transform_matrix.%d.bias" % i]
            th, tc = tt[i][h], tt[i][c]
            NE.append(((S - F.linear(torch.cat([th, tc], 1), Wt, bt)) ** 2).mean(-1).mean(-1))
            tu = TP.user_encoder(P, "teachers.%d." % i, th, mask, cfg["user_log_mask"])
            UE.append(((user - F.linear(tu, Wt, bt)) ** 2).mean(-1))
            ts = torch.bmm(tc, tu[:, :, None])[..., 0]
            ts_all.append(ts)
            tl.append(F.cross_entropy(ts, label, reduction="none"))
        tw = torch.softmax(-torch.stack(tl, -1), -1)
        mix = (torch.stack(ts_all, -1) * tw[:, None, :]).sum(-1)
        tau = cfg["temperature"]
        distill = (-(torch.softmax(mix / tau, -1) * torch.log_softmax(score / tau, -1)).sum(-1)).mean()
        emb = (torch.stack(NE, -1) * tw).sum(-1).mean() + (torch.stack(UE, -1) * tw).sum(-1).mean()
    (distill + cfg["coef"] * target + emb).backward()
    G = {k: (v.grad.numpy() if v.grad is not None else np.zeros(tuple(v.shape), np.float32)) for k, v in P.items() if v.requires_grad}
    if embed:                                     # nn.Embedding(padding_idx=0): the padding row has no gradient (embed_train_ref.py)
        G[EMB_KEYS[0]] = G[EMB_KEYS[0]].copy()
        G[EMB_KEYS[0]][0] = 0.0
    _PORT[key] = (np.array([float(distill.detach()), float(target.detach()), float(emb.detach())], np.float64), score.detach().numpy(), G)
    return _PORT[key]


def against_port(dtype, model, name, teachers, mult=1.0, embed_gtol=None):
    """mult: the fp16 scaler's multiplier the step runs at.  embed_gtol: train_embeddings=True, the five embedding keys held to
    this bound (tests/test_embed_train_gpu.py's), every other key to widths_ref.TOLS as ever."""
    embed = embed_gtol is not None
    ref_l, ref_s, G = port_step(model, name, teachers, embed)
    ltol, stol, gtol = W.TOLS[dtype]
    B = ref_s.shape[0]
    more = dict(train_embeddings=True) if embed else {}
    eng = make(dtype, B, model, teachers, **more)
    assert mult == 1.0 or eng.f16
    eng.scaler.mult = mult
    got = run(eng, name, True, model=model)
    off = run(make(dtype, B, model, teachers, **more), name, False, model=model, backward=False)
    torch.cuda.synchronize()
    assert torch.equal(got["score"], off["score"]), "student_score moved with the option"
    assert (got["count"].cpu().numpy() == R.eligibility(*R.fixture(name)).sum(1)).all()
    le = np.abs(got["losses"][:3].cpu().numpy() - ref_l).max() / max(1.0, np.abs(ref_l).max())
    se = np.abs(got["score"].cpu().numpy() - ref_s).max() / max(1.0, np.abs(ref_s).max())
    emb = []
    if embed:
        from embed_train_ref import EMB_KEYS as emb
        assert set(emb) <= set(eng.grads) and set(emb) <= set(G)
        ew, ek, ebad = V.compare_grads(model, list(emb), lambda k: eng.grad(k).cpu().numpy(), G, embed_gtol)
        print("\n[inbatch %s %s %s] worst embedding gradient %.2e of %.2e (%s)" % (model, name, dtype, ew, embed_gtol, ek[-48:]))
        assert not ebad and np.isfinite(ew), ebad
    worst, wk, bad = V.compare_grads(model, [k for k in eng.grads if k not in emb], lambda k: eng.grad(k).cpu().numpy(), G, gtol)
    print("\n[inbatch %s %s %s teachers %s] loss %.2e score %.2e worst gradient %.2e (%s); target %.4f (plain %.4f)" % (
        model, name, dtype, teachers, le, se, worst, wk[-48:], ref_l[1], float(off["losses"][1])))
    assert le < ltol and se < stol
    assert not bad, ["%s: %.3e" % (k[-60:], W.rel_l2(eng.grad(k).cpu().numpy(), G[k])) for k in bad]
    assert np.isfinite(le + se + worst)


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("teachers", [True, False])
@pytest.mark.parametrize("name", ["e4", "e5"])
def test_a_whole_step_against_autograd(dtype, teachers, name):
    against_port(dtype, "att", name, teachers)


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_mean_pooling_against_autograd(dtype):
    """mean pooling and user_log_mask (variants_ref's mean_ulm): the port follows both."""
    against_port(dtype, "mean_ulm", "e5", True)


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_nrms_long_lived_engine_equals_a_fresh_one(dtype):
    """The port has no NRMS user encoder.  A long-lived cls_nrms engine - on, another batch on, off, then the first batch on again -
    must give the fresh engine's bits, and its loss must be the reference's on the engine's own user and candidate rows."""
    eng = make(dtype, 5, "cls_nrms")
    first = run(eng, "e5", True, model="cls_nrms")
    run(eng, "e5b", True, model="cls_nrms")
    run(eng, "e5", False, model="cls_nrms")
    again = run(eng, "e5", True, model="cls_nrms")
    N = 5 * (HR.U + HR.C)
    S = eng.S.clone()
    fresh = run(make(dtype, 5, "cls_nrms"), "e5", True, model="cls_nrms")
    torch.cuda.synchronize()
    assert not same(first, fresh) and not same(again, fresh) and torch.equal(again["count"], fresh["count"])
    h, c, _, y = R.engine_feed("e5")
    ref = R.loss(S[N:N + 5].cpu().numpy(), S[5 * HR.U:N].cpu().numpy(), again["score"].cpu().numpy(), y, R.eligibility(h, c), 0.3)
    assert abs(float(again["losses"][1]) - ref["target"]) <= 1e-4 * abs(ref["target"])      # the kernel tests' FWD bound


# ---------------------------------------------------------------------------------------------------------------- step forms
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_dedup_plan_changes_no_bit_of_the_loss(dtype):
    """With a de-duplication plan and without: losses, scores and counts have equal bits (the logits are taken from slot rows
    either way); the gradients are sums in another order, within the gradient tolerance of each other."""
    h, c, _, _ = R.engine_feed("e5")
    plan = build_plan(h, c, quantum=64)
    assert plan is not None and plan.n_enc == 64
    a = run(make(dtype, 5), "e5", True)
    eng = make(dtype, 5)
    b = run(eng, "e5", True, plan=plan.to(DEV))
    torch.cuda.synchronize()
    assert not same(a, b, ("losses", "score", "count"))
    ref = make(dtype, 5)
    ref.flat_g.copy_(a["flat_g"])
    G = {k: ref.grad(k).cpu().numpy() for k in ref.grads}
    worst, wk, bad = V.compare_grads("att", list(eng.grads), lambda k: eng.grad(k).cpu().numpy(), G, W.TOLS[dtype][2])
    assert not bad, (bad, worst, wk)


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_token_feed_equals_indexed_feed(dtype):
    a = run(make(dtype, 4), "e4", True, form="idx")
    b = run(make(dtype, 4), "e4", True, form="tok")
    torch.cuda.synchronize()
    assert not same(a, b, ("losses", "score", "flat_g", "count"))


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_accumulation_window_is_the_sum_of_its_backwards(dtype):
    g0 = run(make(dtype, 5), "e5", True)["flat_g"]
    g1 = run(make(dtype, 5), "e5b", True)["flat_g"]
    eng = make(dtype, 5)
    run(eng, "e5", True, micro=(0, 2))
    win = run(eng, "e5b", True, micro=(1, 2))
    torch.cuda.synchronize()
    assert torch.equal(win["flat_g"], g0 + g1)


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_short_batch_and_back(dtype):
    """B = 5 -> 3 -> 5 on one engine: the buffers follow the workspace's re-lay, every step equals a fresh engine's."""
    eng = make(dtype, 5)
    for name, B in (("e5", 5), ("e3", 3), ("e5b", 5)):
        got = run(eng, name, True)
        assert eng._inbatch["dz"].shape == (B, B * HR.C)
        want = run(make(dtype, B), name, True)
        torch.cuda.synchronize()
        assert not same(got, want, ("losses", "score", "flat_g", "count")), (name, same(got, want))


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_one_impression_is_the_plain_step(dtype):
    """B = 1: no foreign slot, so the loss is the plain one - within the tolerances, not bit for bit (the target's arithmetic
    differs: another kernel, another order)."""
    ltol, _, gtol = W.TOLS[dtype]
    eng = make(dtype, 1)
    on = run(eng, "e4", True, B=1)
    ref = make(dtype, 1)
    off = run(ref, "e4", False, B=1)
    torch.cuda.synchronize()
    assert int(on["count"][0]) == 0 and torch.equal(on["score"], off["score"])
    lo, lf = on["losses"][:3].cpu().numpy().astype(np.float64), off["losses"][:3].cpu().numpy().astype(np.float64)
    assert np.abs(lo - lf).max() / max(1.0, np.abs(lf).max()) < ltol
    G = {k: ref.grad(k).cpu().numpy() for k in ref.grads}
    worst, wk, bad = V.compare_grads("att", list(eng.grads), lambda k: eng.grad(k).cpu().numpy(), G, gtol)
    assert not bad, (bad, worst, wk)


def test_refusals():
    """stage1=True has no users; a token feed carries no ids of its own."""
    s = _shared("att")
    h, c, m, y = dfeed("e4")
    s1 = E.Engine(E.EngineConfig(**dict(V.engine_kwargs("att"), stage1=True)), DEV, max_batch=4)
    with pytest.raises(ValueError, match="stage1"):
        s1.forward(None, m, None, y, teacher_tables=s["tables"], t_hidx=h, t_cidx=c, news_combined=s["comb"], inbatch_ids=(h, c))
    eng = make("fp16", 4)
    tok = (s["comb"][h.long()].long(), m, s["comb"][c.long()].long(), y, [s["tables"][i][h.long()] for i in range(HR.T_)],
           [s["tables"][i][c.long()] for i in range(HR.T_)])
    with pytest.raises(ValueError, match="inbatch_ids"):
        eng.forward(*tok, inbatch_ids=True)
    with pytest.raises(ValueError, match="inbatch_ids"):
        eng.forward(*tok, inbatch_ids=(h[:3], c[:3]))
    assert eng._inbatch is None


# ---------------------------------------------------------------------------------------------------------------- run.py
def test_run_py_trains_with_the_flag(tmp_path):
    """run.py --mode train --synthetic True --inbatch_negatives True in a child process, a handful of steps at a tiny shape: it
    ends with finite losses, logs the eligible count on the log steps, and records the flag beside the optimiser state."""
    import math
    import os
    import re
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pkg = os.path.join(root, "tiny-newsrec_amd")
    cmd = [sys.executable, "-u", os.path.join(pkg, "run.py"), "--mode", "train", "--synthetic", "True", "--inbatch_negatives", "True",
           "--epochs", "1", "--max_steps_per_epoch", "4", "--log_steps", "2", "--enable_hvd", "False", "--batch_size", "4",
           "--num_words_title", "30", "--news_dim", "256", "--num_student_layers", "2", "--bert_trainable_layer", "1",
           "--num_teachers", "2", "--user_log_mask", "False", "--model", "NAML", "--model_type", "tnlrv3", "--save_optimizer", "True",
           "--model_dir", str(tmp_path)]
    r = subprocess.run(cmd, env=dict(os.environ, PYTHONPATH=pkg), capture_output=True, text=True, timeout=600, cwd=pkg)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    counts = [float(x) for x in re.findall(r"in-batch negatives: ([0-9.]+) eligible per impression", out)]
    losses = [float(x) for x in re.findall(r"train_loss: ([-0-9.a-z]+)", out)]
    assert len(counts) == 2 and all(0.0 < x <= 3 * 5 for x in counts), out[-2000:]          # steps 0 and 2 of four; B = 4, C = 5
    assert len(losses) == 2 and all(math.isfinite(x) for x in losses), out[-2000:]
    ck = torch.load(str(tmp_path / "epoch-1.pt"), map_location="cpu")
    assert ck["train_state"]["flags"]["inbatch_negatives"] is True
