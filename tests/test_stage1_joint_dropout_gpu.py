"""Stage 1's joint passes in train mode (hidden / attention-probability dropout live, as Post-train_KD.ipynb cell 19 runs them):
every pass keeps its own forward-call number and draws the per-pass form's masks (the split sites of tnr_gemm_nt_do_split /
tnr_ln_bwd_do_split at the pass boundary), so news vectors, scores and losses are bit-identical to joint = False under the same
seed and the parameter gradients are the same sums in another order."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import load_stage1_case        # noqa: E402
from oracle import newsrec_oracle as O      # noqa: E402
from stage1 import Stage1Engine             # noqa: E402

DEV = "cuda:0"
TOL = {"bf16": 1.6e-2, "fp16": 1e-3}
GTOL = {"bf16": 6e-2, "fp16": 1.5e-2}
SEED = 4242


def _make(z, cfg, dtype):
    seed, B, T_, C, Lt, Lb, D, A, nl = [int(x) for x in z["meta"]]
    eng = Stage1Engine(n_layers=nl, trainable_layers=cfg["trainable_layers"], num_teachers=T_, npratio=C - 1, title_len=Lt,
                       body_len=Lb, device=DEV, batch=B, dtype=dtype, news_dim=D)
    return eng, B


def _dev(inp):
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    title, body, label, tt, tb = inp
    return t(title), t(body), t(label), [t(x) for x in tt], [t(x) for x in tb]


def _step(eng, fwd):
    """One forward + backward from forward call 0 of both passes -> (flat_g, losses, S, score)."""
    eng.title.drop_calls = eng.body.drop_calls = 0
    eng.title.flat_g.fill_(float("nan"))
    eng.title.S.fill_(float("nan"))
    fwd()
    eng.backward()
    torch.cuda.synchronize()
    B, N, Rt = eng.cur
    t = eng.title
    return t.flat_g.clone(), t.losses.clone(), t.S[:Rt].clone(), t.score[:B].clone()


def _compare(eng, joint, per_pass, bound=2e-5):
    for k in (1, 2, 3):
        assert bool(torch.isfinite(joint[k]).all()), k
        assert torch.equal(joint[k], per_pass[k]), k
    t = eng.title
    worst = 0.0
    for name, gk in t.grads.items():
        o = gk.storage_offset() - t.flat_g.storage_offset()
        va, vb = joint[0][o:o + gk.numel()], per_pass[0][o:o + gk.numel()]
        assert bool(torch.isfinite(va).all()), name                  # every gradient was written (flat_g was all NaN)
        e = float((va - vb).norm()) / max(float(vb.norm()), 1e-30)
        worst = max(worst, e)
        assert e <= bound, (name, e)
    return worst


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("case", ["stage1_cfg4.npz", "stage1_full.npz"])
def test_joint_passes_with_dropout_equal_the_per_pass_form(dtype, case):
    z, P, cfg, inp = load_stage1_case(case)
    eng, B = _make(z, cfg, dtype)
    eng.load_state_dict(P)
    eng.set_dropout(0.1, 0.1, SEED)
    d = _dev(inp)
    res = {}
    for joint in (False, True):
        eng.joint = joint
        res[joint] = _step(eng, lambda: eng.forward(*d))
        assert eng.ran_joint == joint
    worst = _compare(eng, res[True], res[False])
    # the masks are live: eval mode gives other vectors
    eng.set_dropout(0.0, 0.0, SEED)
    ev = _step(eng, lambda: eng.forward(*d))
    assert eng.ran_joint and not torch.equal(ev[2], res[True][2])
    print("\n[stage1 joint + dropout %s %s] worst relative L2 gap of a parameter gradient to the per-pass form: %.2e" % (case, dtype, worst))


def test_rewinding_the_call_counter_reproduces_a_joint_step():
    z, P, cfg, inp = load_stage1_case("stage1_cfg4.npz")
    eng, B = _make(z, cfg, "fp16")
    eng.load_state_dict(P)
    eng.set_dropout(0.1, 0.1, SEED)
    d = _dev(inp)
    a = _step(eng, lambda: eng.forward(*d))
    assert eng.ran_joint
    eng.forward(*d)                                   # the next forward call draws new masks ...
    assert not torch.equal(eng.title.score[:B], a[3])
    eng.backward()
    b = _step(eng, lambda: eng.forward(*d))          # ... and call 0 again the same ones, in the backward too
    for x, y in zip(a, b):
        assert torch.equal(torch.nan_to_num(x), torch.nan_to_num(y))


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_train_mode_golden_holds_on_the_joint_path(dtype):
    """stage1_cfg4_drop.npz (the notebook's DistillModel under the same masks, and the oracle) on the joint passes."""
    from oracle import dropout_oracle as DO
    z, P, cfg, inp = load_stage1_case("stage1_cfg4_drop.npz")
    p_h, p_a, seed = float(z["dropout"][0]), float(z["dropout"][1]), int(z["dropout"][2])
    eng, B = _make(z, cfg, dtype)
    eng.load_state_dict(P)
    eng.set_dropout(p_h, p_a, seed)
    losses, score = eng.forward(*_dev(inp))
    assert eng.ran_joint
    eng.backward()
    torch.cuda.synchronize()
    tol = TOL[dtype]
    l = losses.cpu().numpy()
    got = dict(distill=l[0], target=l[1], emb=l[2], total=float(eng.total_loss().item()))
    for k in got:
        assert abs(got[k] - float(z[k])) <= tol * max(1.0, abs(float(z[k]))), k
    assert np.abs(score.cpu().numpy() - z["score"]).max() <= tol * max(1.0, np.abs(z["score"]).max())
    out = O.distill_fwd(P, cfg, *inp, drop_title=DO.Dropout(p_h, p_a, seed, 0), drop_body=DO.Dropout(p_h, p_a, seed, 1))
    G = O.distill_bwd(P, cfg, out)
    for k in eng.title.grads:
        ref, g = G[k], eng.grad(k).cpu().numpy()
        if k.endswith("self.key.bias") or k.endswith("att_fc2.bias"):
            assert np.abs(g).max() < 1e-3
            continue
        rn = np.sqrt((ref.astype(np.float64) ** 2).sum())
        err = np.sqrt(((g - ref).astype(np.float64) ** 2).sum()) / (rn + 1e-12)
        assert err < GTOL[dtype], "%s: relative L2 error %.3e" % (k, err)
        gn = float(z["gnorm." + k])
        assert abs(np.sqrt((g.astype(np.float64) ** 2).sum()) - gn) <= GTOL[dtype] * gn + 1e-7, k


@pytest.mark.parametrize("Lt,Lb,Kn", [(30, 128, 4), (24, 512, 9)])       # bench.py's two stage-1 shapes
def test_bench_shapes_with_dropout_joint_equals_per_pass(Lt, Lb, Kn):
    """B = 32, 2-layer student, 4 teachers: the joint M (8 896 / 24 064 rows) puts the pass boundary inside a tile of the
    persistent kernels."""
    import hashinit
    import synth
    nl, T_, B, nd = 2, 4, 32, 3000
    eng = Stage1Engine(n_layers=nl, trainable_layers=(0, 1), num_teachers=T_, npratio=Kn, title_len=Lt, body_len=Lb, device=DEV, batch=B,
                       dtype="fp16")
    eng.load_state_dict({k: torch.from_numpy(hashinit.init_tensor(1234, k, tuple(sh))) for k, sh in eng.shapes.items()})
    eng.set_dropout(0.1, 0.1, SEED)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    d_title, d_body = t(synth.news_table(11, nd - 1, Lt)), t(synth.news_table(12, nd - 1, Lb, mean_len=0.6 * Lb, std_len=0.25 * Lb))
    d_tt = t(synth.teacher_tables(13, T_, nd - 1, eng.cfg_t.D))
    d_tb = t(synth.teacher_tables(14, T_, nd - 1, eng.cfg_t.D))
    rs = np.random.RandomState(1234)
    pidx, label = t(rs.randint(1, nd, (B, 1 + Kn)).astype(np.int32)), t(rs.randint(0, 1 + Kn, B).astype(np.int64))
    res = {}
    for joint in (False, True):
        eng.joint = joint
        res[joint] = _step(eng, lambda: eng.forward_indexed(d_title, d_body, pidx, label, d_tt, d_tb))
        assert eng.ran_joint == joint
    worst = _compare(eng, res[True], res[False])
    print("\n[stage1 bench shape %d / %d + dropout] worst relative L2 gap of a parameter gradient to the per-pass form: %.2e" % (Lt, Lb, worst))


def test_joint_training_with_dropout_follows_the_per_pass_form():
    """Eight train-mode optimiser steps, a short last batch and one more step of the joint passes against the per-pass form from the
    same start and seed: the first step's losses bit for bit, the rest within 1e-3 (gradients differ in fp32 summation order only)."""
    z, P, cfg, inp = load_stage1_case("stage1_cfg4.npz")
    d = _dev(inp)
    res = []
    for joint in (False, True):
        eng, B = _make(z, cfg, "fp16")
        eng.joint = joint
        eng.load_state_dict(P)
        eng.set_dropout(0.1, 0.1, SEED)
        ls = []
        for i in range(8):
            eng.forward(*d)
            assert eng.ran_joint == joint
            ls.append(eng.title.losses.clone())
            eng.backward()
            eng.step(1e-4, lr_bert=1e-5)
        half = (d[0][:B // 2], d[1][:B // 2], d[2][:B // 2], [x[:B // 2] for x in d[3]], [x[:B // 2] for x in d[4]])
        eng.forward(*half)
        assert eng.ran_joint == joint
        ls.append(eng.title.losses.clone())
        eng.backward()
        eng.step(1e-4, lr_bert=1e-5)
        eng.forward(*d)
        ls.append(eng.title.losses.clone())
        torch.cuda.synchronize()
        res.append(torch.stack(ls).cpu().numpy())
    assert np.array_equal(res[0][0], res[1][0])
    assert np.isfinite(res[1]).all()
    np.testing.assert_allclose(res[1], res[0], rtol=0, atol=1e-3)


def test_joint_ok_falls_back_when_the_grouped_weight_gradients_cannot_tile():
    """inter = 128 * odd: the shared-round _wgrad_flush's 256 x 256 tiles do not fit - the step runs per pass instead of asserting."""
    eng = Stage1Engine(n_layers=2, trainable_layers=(0, 1), num_teachers=2, npratio=1, title_len=16, body_len=64, device=DEV, batch=2,
                       dtype="fp16", hidden=256, heads=4, inter=384, news_dim=64)
    import hashinit
    eng.load_state_dict({k: torch.from_numpy(hashinit.init_tensor(7, k, tuple(sh))) for k, sh in eng.shapes.items()})
    eng.set_dropout(0.1, 0.1, SEED)
    B, C = 2, 2
    rs = np.random.RandomState(0)
    ids = lambda n, L: np.concatenate([rs.randint(1, 1000, (n, L)), np.ones((n, L), np.int64)], 1)
    title = torch.from_numpy(ids(B * C, 16).reshape(B, C, 32)).to(DEV)
    body = torch.from_numpy(ids(B, 64)).to(DEV)
    label = torch.zeros(B, dtype=torch.int64, device=DEV)
    tt = [torch.randn(B, C, 64, device=DEV) for _ in range(2)]
    tb = [torch.randn(B, 64, device=DEV) for _ in range(2)]
    eng.forward(title, body, label, tt, tb)
    assert not eng.ran_joint
    eng.backward()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(eng.title.losses[:3]).all())


def test_post_train_kd_train_mode_logs_the_joint_form(tmp_path):
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONPATH=os.path.join(root, "tiny-newsrec_amd"))
    cmd = [sys.executable, "-u", os.path.join(root, "tiny-newsrec_amd", "post_train_kd.py"), "--synthetic", "True", "--enable_hvd",
           "False", "--max_steps", "3", "--log_steps", "1", "--num_hidden_layers", "2", "--bert_trainable_layer", "0", "1",
           "--num_teachers", "2", "--npratio", "3", "--batch_size", "4", "--max_body_len", "128", "--synthetic_docs", "300",
           "--save_dir", str(tmp_path)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900, cwd=os.path.join(root, "tiny-newsrec_amd"))
    out = r.stdout + r.stderr
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert "train-mode dropout" in out and "stage 1: joint passes" in out, out[-3000:]
    assert out.count("stage 1: joint passes") == 1 and "per-pass" not in out
    assert "d_loss" in out and "nan" not in out.lower()
