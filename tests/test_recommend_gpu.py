"""GPU: Engine.topk / Engine.recommend and `run.py --mode recommend` on the golden tiny data path (tests/test_n2_gpu.py's
setup): against the oracle's user vectors, against the scores run.test collects for the same impressions, the history
exclusion, the output file, and that a recommend call between two training steps changes no bit of the second."""
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import engine as E                        # noqa: E402
import topk_ref as R                      # noqa: E402
from helpers import load_case             # noqa: E402
from oracle import data_oracle as DO      # noqa: E402
from oracle import newsrec_oracle as O    # noqa: E402
import hashinit                           # noqa: E402
from helpers import FULL, GOLDEN, state_shapes   # noqa: E402

DEV = "cuda:0"
U = 50


def _setup():
    """tests/test_n2_gpu.py's: the golden tokenised titles (41 rows incl. the padding row 0) and a frozen 2-layer student."""
    import os
    z = np.load(os.path.join(GOLDEN, "datapath.npz"))
    comb = z["news_combined"].astype(np.int32)
    P = hashinit.init_state_dict(7, state_shapes(FULL, 2, 256, 0))
    eng = E.Engine(E.EngineConfig(n_layers=2, trainable_layers=(), num_teachers=0, user_log_mask=True), DEV, max_batch=4)
    eng.load_state_dict(P)
    return z, comb, P, eng


def _lines():
    """The behaviours lines of test_n2_gpu.test_run_test_mode_end_to_end (ids N41 .. N43 are not in the table: row 0)."""
    rs = np.random.RandomState(3)
    lines = []
    for j in range(9):
        hist = " ".join("N%d" % rs.randint(1, 41) for _ in range(rs.randint(0, 60)))
        labs = rs.randint(0, 2, rs.randint(2, 12))
        imp = " ".join("N%d-%d" % (rs.randint(1, 44), l) for l in labs)
        lines.append("%d\tU%d\tt\t%s\t%s" % (j, j, hist, imp))
    return lines


def _hist(news_index, lines):
    H, M = [], []
    for ln in lines:
        h, m = DO.pad_to_fix_len(DO.trans_to_nindex(news_index, ln.split("\t")[3].split()), U)
        H.append(h)
        M.append(m)
    return np.asarray(H, np.int32), np.asarray(M, np.float32)


def _recommend_all(eng, ns, H, M, k, exclude_history):
    """Engine.recommend in batches of the engine's capacity -> numpy (idx, score)."""
    I, S = [], []
    for b in range(0, len(H), eng.B_alloc):
        i, s = eng.recommend(ns, torch.from_numpy(H[b:b + eng.B_alloc]).to(DEV), torch.from_numpy(M[b:b + eng.B_alloc]).to(DEV), k,
                             exclude_history=exclude_history)
        I.append(i.cpu().numpy())
        S.append(s.cpu().numpy())
    return np.concatenate(I), np.concatenate(S)


@pytest.fixture(scope="module")
def world():
    z, comb, P, eng = _setup()
    news_index = {str(k): int(v) for k, v in zip(z["news_ids"], z["news_index"])}
    ns = eng.encode_news(torch.from_numpy(comb).to(DEV))
    lines = _lines()
    H, M = _hist(news_index, lines)
    return types.SimpleNamespace(z=z, comb=comb, P=P, eng=eng, news_index=news_index, ns=ns, ns_host=ns.cpu().numpy(), lines=lines, H=H, M=M)


def test_recommend_against_the_oracles_user_vectors(world):
    w = world
    Nn = w.ns_host.shape[0]
    for k, excl in ((5, True), (Nn - 1, False), (Nn + 3, True)):
        idx, sc = _recommend_all(w.eng, w.ns, w.H, w.M, k, excl)
        ex = w.H if excl else None
        # the engine's own user vectors: the kernel's contract, fp32 bound only
        uv = np.concatenate([w.eng.user_vectors(w.ns, torch.from_numpy(w.H[b:b + 4]).to(DEV), torch.from_numpy(w.M[b:b + 4]).to(DEV)).cpu().numpy()
                             for b in range(0, len(w.H), 4)])
        R.check_result(uv, w.ns_host, ex, 1, k, idx, sc)
        # the oracle's user vectors on the same table: the engine's agree with them to rtol 1e-4 / atol 1e-5 (the bound
        # tests/test_n2_gpu.py holds these vectors to), which moves a score by at most sum_k (1e-4 |u_k| + 1e-5) |n_k|
        ref_u, _ = O.user_encoder_fwd(w.P, "student.user_encoder.", w.ns_host[w.H], w.M, True)
        s64 = R.scores64(ref_u, w.ns_host)
        slack = R.bound(ref_u, w.ns_host) + (1e-4 * np.abs(ref_u).astype(np.float64) + 1e-5) @ np.abs(w.ns_host).astype(np.float64).T
        ok = R.eligible(s64, ex, 1)
        ridx, _ = R.topk_ref(ref_u, w.ns_host, ex, 1, k)
        assert np.array_equal(idx >= 0, ridx >= 0)
        for u in range(len(w.H)):
            r = idx[u][idx[u] >= 0]
            assert ok[u, r].all() and len(set(r)) == len(r)
            assert (np.abs(sc[u, :len(r)] - s64[u, r]) <= slack[u, r]).all()
            rest = ok[u].copy()
            rest[r] = False
            if len(r):
                assert not (s64[u, rest] > s64[u, r[-1]] + slack[u, rest] + slack[u, r[-1]]).any()


def test_full_ranking_agrees_with_test_mode_and_history_is_excluded(world, tmp_path, monkeypatch):
    import run
    w = world
    Nn = w.ns_host.shape[0]
    d = tmp_path / "test"
    d.mkdir()
    (d / "behaviors_0.tsv").write_text("\n".join(w.lines) + "\n")
    torch.save({"model_state_dict": {k: torch.from_numpy(v) for k, v in w.P.items()}, "category_dict": {}, "word_dict": None,
                "subcategory_dict": {}}, str(tmp_path / "epoch-1.pt"))
    monkeypatch.setattr(run, "_news_table", lambda a, dd, mode: (w.news_index, w.comb))
    per = []
    run.test(_args(tmp_path, d), collect=per)
    idx, sc = _recommend_all(w.eng, w.ns, w.H, w.M, Nn - 1, False)
    assert (np.sort(idx, axis=1) == np.arange(1, Nn)).all()                       # every real row, once
    uv = np.concatenate([w.eng.user_vectors(w.ns, torch.from_numpy(w.H[b:b + 4]).to(DEV), torch.from_numpy(w.M[b:b + 4]).to(DEV)).cpu().numpy()
                         for b in range(0, len(w.H), 4)])
    bd = R.bound(uv, w.ns_host)
    checked = 0
    for u, (ln, (got_sc, _)) in enumerate(zip(w.lines, per)):
        c = np.asarray(DO.trans_to_nindex(w.news_index, [i.split("-")[0] for i in ln.split("\t")[4].split()]))
        pos = np.full(Nn, -1)
        pos[idx[u]] = np.arange(Nn - 1)
        for a in range(len(c)):
            for b in range(len(c)):
                # collect's score of a clearly above b's (by more than the two fp32 bounds): a is ranked before b
                if c[a] >= 1 and c[b] >= 1 and got_sc[a] - got_sc[b] > bd[u, c[a]] + bd[u, c[b]]:
                    assert pos[c[a]] < pos[c[b]], (u, c[a], c[b])
                    checked += 1
    assert checked > 50
    # exclude_history removes exactly the clicked rows and keeps the others in their order
    idx_x, sc_x = _recommend_all(w.eng, w.ns, w.H, w.M, Nn - 1, True)
    for u in range(len(w.H)):
        clicked = set(int(x) for x in w.H[u] if x >= 1)
        keep = [i for i, x in enumerate(idx[u]) if int(x) not in clicked]
        assert np.array_equal(idx_x[u, :len(keep)], idx[u, keep]) and (idx_x[u, len(keep):] == -1).all()
        assert np.array_equal(sc_x[u, :len(keep)].view(np.int32), sc[u, keep].view(np.int32)) and np.isneginf(sc_x[u, len(keep):]).all()
    assert any(len(set(int(x) for x in h if x >= 1)) > 0 for h in w.H)


def _args(model_dir, data_dir, **kw):
    return types.SimpleNamespace(enable_hvd=False, enable_gpu=True, model_dir=str(model_dir), load_ckpt_name="epoch-1.pt",
                                 test_data_dir=str(data_dir), filename_pat="behaviors_*.tsv", batch_size=4, npratio=4,
                                 user_log_length=U, shuffle_buffer_size=100, num_teachers=0, num_student_layers=2,
                                 bert_trainable_layer=[], config_name=None, pooling="att", model="NAML", news_dim=256,
                                 news_query_vector_dim=200, user_query_vector_dim=200, num_words_title=30,
                                 user_log_mask=True, temperature=1.0, coef=1.0, num_teacher_layers=12, log_steps=1, dtype="fp16", **kw)


@pytest.mark.parametrize("exclude_history", [True, False])
def test_recommend_mode_end_to_end(world, tmp_path, monkeypatch, exclude_history):
    import run
    w = world
    d = tmp_path / "test"
    d.mkdir()
    (d / "behaviors_0.tsv").write_text("\n".join(w.lines[:5]) + "\n")
    (d / "behaviors_1.tsv").write_text("\n".join(w.lines[5:]) + "\n")
    torch.save({"model_state_dict": {k: torch.from_numpy(v) for k, v in w.P.items()}, "category_dict": {}, "word_dict": None,
                "subcategory_dict": {}}, str(tmp_path / "epoch-1.pt"))
    monkeypatch.setattr(run, "_news_table", lambda a, dd, mode: (w.news_index, w.comb))
    out, n = run.recommend(_args(tmp_path, d, top_k=7, recommend_out=None, exclude_history=exclude_history, use_ema=False))
    assert n == 9 and out == str(tmp_path / "recommend.tsv")
    got = open(out).read().split("\n")
    assert got[-1] == "" and len(got) == 10
    idx, sc = _recommend_all(w.eng, w.ns, w.H, w.M, 7, exclude_history)
    nid_of = {v: k for k, v in w.news_index.items()}
    for u, (ln, g) in enumerate(zip(w.lines, got)):
        f = g.split("\t")
        assert f[:2] == ln.split("\t")[:2] and len(f) == 3
        pairs = [p.rsplit(":", 1) for p in f[2].split()]
        want = [(nid_of[int(i)], "%.6g" % s) for i, s in zip(idx[u], sc[u]) if i >= 0]
        assert [(a, b) for a, b in pairs] == want and len(want) == 7


def test_recommend_between_two_training_steps_changes_nothing():
    z, P, cfg, inp = load_case("full_model_0.npz")
    T_ = len(inp[4])
    seed, B, _, Uc, C, L, D, A, nl = [int(x) for x in z["meta"]]
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    rs = np.random.RandomState(1)
    table = t(rs.randn(300, D).astype(np.float32))
    hidx = t(rs.randint(0, 300, (B, Uc)).astype(np.int32))
    hmask = t((rs.rand(B, Uc) > 0.3).astype(np.float32))
    outs = []
    for with_call in (False, True):
        eng = E.Engine(E.EngineConfig(n_layers=nl, trainable_layers=cfg["trainable_layers"], num_teachers=T_, user_log_length=Uc,
                                      npratio=C - 1, num_words=L, news_dim=D, user_log_mask=cfg["user_log_mask"],
                                      temperature=cfg["temperature"], coef=cfg["coef"]), DEV, max_batch=B)
        eng.load_state_dict(P)
        step = lambda: (eng.forward(t(inp[0]), t(inp[1]), t(inp[2]), t(inp[3]), [t(x) for x in inp[4]], [t(x) for x in inp[5]]),
                        eng.backward(), eng.step(lr=1e-3))[0]
        step()
        if with_call:
            idx, sc = eng.recommend(table, hidx, hmask, 10)
            assert (idx.cpu().numpy() >= 1).all() and torch.isfinite(sc).all()
        else:
            assert not eng._topk_ws                                              # nothing allocated unless it is called
        losses, score = step()
        torch.cuda.synchronize()
        outs.append((losses.cpu().numpy().copy(), score.cpu().numpy().copy(), eng.flat[True].cpu().numpy().copy(), eng.step_count))
    for a, b in zip(outs[0][:3], outs[1][:3]):
        assert np.array_equal(a.view(np.int32), b.view(np.int32))
    assert outs[0][3] == outs[1][3]
