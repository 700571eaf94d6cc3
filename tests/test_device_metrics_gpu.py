"""GPU: run.test with device_metrics=True against its default host loop on the same file, and Engine.evaluate's footprint.
The set-up is tests/test_n2_gpu.py's: 41 real tokenised titles, hash-initialised 2-layer weights, a generated behaviours file."""
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import metrics                              # noqa: E402
from test_n2_gpu import DEV, _setup         # noqa: E402


@pytest.fixture(scope="module")
def both(tmp_path_factory):
    """run.test twice on one file: the default path and the device path -> their (sums, n_local, cnt_metric, collected)."""
    import run
    tmp_path = tmp_path_factory.mktemp("device_metrics")
    z, comb, P, eng = _setup()
    del eng
    news_index = {str(k): int(v) for k, v in zip(z["news_ids"], z["news_index"])}
    rs = np.random.RandomState(3)
    lines = []
    for j in range(23):
        hist = " ".join("N%d" % rs.randint(1, 41) for _ in range(rs.randint(0, 60)))
        # an impression lists a news once (N41, not in the table, is the one way to row 0): two equal scores with unlike labels
        # would leave MRR and nDCG to the order numpy's argsort happens to give ties, which metrics.py does not fix (its SIMD
        # sorts are not stable); the tie rule itself is tests/test_rankmetrics_kernels_gpu.py's
        n = 1 if j == 9 else rs.randint(2, 12)
        news = rs.permutation(41)[:n] + 1
        labs = rs.randint(0, 2, n)
        if j == 4:
            labs[:] = 0                       # skipped: no positive
        if j == 11:
            labs[:] = 1                       # skipped: no negative
        lines.append("%d\tU%d\tt\t%s\t%s" % (j, j, hist, " ".join("N%d-%d" % (c, l) for c, l in zip(news, labs))))
    d = tmp_path / "test"
    d.mkdir()
    (d / "behaviors_0.tsv").write_text("\n".join(lines) + "\n")
    torch.save({"model_state_dict": {k: torch.from_numpy(v) for k, v in P.items()}, "category_dict": {}, "word_dict": None,
                "subcategory_dict": {}}, str(tmp_path / "epoch-1.pt"))
    mp = pytest.MonkeyPatch()
    mp.setattr(run, "_news_table", lambda a, dd, mode: (news_index, comb))
    out = {}
    try:
        for name, flag in (("host", {}), ("device", {"device_metrics": True})):
            args = types.SimpleNamespace(enable_hvd=False, enable_gpu=True, model_dir=str(tmp_path), load_ckpt_name="epoch-1.pt",
                                         test_data_dir=str(d), filename_pat="behaviors_*.tsv", batch_size=4, npratio=4,
                                         user_log_length=50, shuffle_buffer_size=100, num_teachers=0, num_student_layers=2,
                                         bert_trainable_layer=[], config_name=None, pooling="att", model="NAML", news_dim=256,
                                         news_query_vector_dim=200, user_query_vector_dim=200, num_words_title=30,
                                         user_log_mask=True, temperature=1.0, coef=1.0, num_teacher_layers=12, log_steps=1,
                                         dtype="fp16", **flag)
            per = []
            out[name] = run.test(args, collect=per) + (per,)
    finally:
        mp.undo()
    return out


def test_device_path_counts_and_scores_match_the_host_path(both):
    (hs, hn, hm, hper), (ds, dn, dm, dper) = both["host"], both["device"]
    scored = sum(1 for _, y in hper if 0 < np.asarray(y).mean() < 1)
    assert hn == dn == 23 and hm == dm == scored and 15 <= scored <= 20 and len(hper) == len(dper) == 23
    err = 0.0
    for (a, ya), (b, yb) in zip(hper, dper):
        assert a.shape == b.shape and b.dtype == np.float32 and (np.asarray(ya) == np.asarray(yb)).all()
        if len(a):
            err = max(err, float((np.abs(b - a) / np.maximum(1.0, np.abs(a))).max()))
    print("\n[device metrics] scores against the host path's: max |err| / max(1, |ref|) %.2e" % err)
    assert err <= 1e-3, err


def test_device_sums_are_metrics_py_on_the_devices_own_scores(both):
    """Near-ties between the two score routes can flip a rank (tests/test_n2_gpu.py's comment (b)), so the sums are held to
    metrics.py applied to the scores the device itself produced: 1e-12 per impression."""
    ds, dn, dm, dper = both["device"]
    want, cnt = np.zeros(4), 0
    for s, y in dper:
        y = np.asarray(y)
        if y.mean() in (0, 1):
            continue
        want += [metrics.roc_auc_score(y, s), metrics.mrr_score(y, s), metrics.ndcg_score(y, s, 5), metrics.ndcg_score(y, s, 10)]
        cnt += 1
    assert cnt == dm
    print("\n[device metrics] sums %s, metrics.py on the same scores %s" % (ds, want))
    assert (np.abs(np.asarray(ds) - want) <= 1e-12 * dn).all()


def test_evaluate_leaves_the_engine_as_user_vectors_does():
    z, comb, P, eng = _setup()
    ns = eng.encode_news(torch.from_numpy(comb).to(DEV))
    rs = np.random.RandomState(0)
    hidx = torch.from_numpy(rs.randint(0, 41, (3, 50)).astype(np.int32)).to(DEV)
    mask = torch.from_numpy((rs.rand(3, 50) > 0.5).astype(np.float32)).to(DEV)
    cands = [rs.randint(0, 41, n) for n in (5, 1, 70)]
    labels = [np.array([1, 0, 0, 1, 0]), np.array([1]), (np.arange(70) % 7 == 0).astype(np.int64)]

    def state():
        torch.cuda.synchronize()
        bufs = {k: v.clone() for k, v in vars(eng).items() if isinstance(v, torch.Tensor)}
        scal = {k: v for k, v in vars(eng).items() if isinstance(v, (int, float, bool, type(None)))}
        return bufs, scal

    uv = eng.user_vectors(ns, hidx, mask)
    b0, s0 = state()
    acc, scores, per = eng.evaluate(ns, hidx, mask, cands, labels, per=True)
    b1, s1 = state()
    assert s0 == s1 and sorted(b0) == sorted(b1) and len(b0) > 20
    for k in b0:
        assert torch.equal(b0[k], b1[k]) or (torch.isnan(b0[k]) == torch.isnan(b1[k])).all() and \
            torch.equal(torch.nan_to_num(b0[k].float()), torch.nan_to_num(b1[k].float())), k
    assert acc.dtype == torch.float64 and acc.shape == (6,) and scores.shape == (76,) and per.shape == (3, 4)
    assert acc.cpu().tolist()[:2] == [3.0, 2.0]
    # the scores are the user vectors' against the listed rows, and a second call adds to acc
    want = torch.cat([ns[torch.from_numpy(c).to(DEV).long()] @ uv[b] for b, c in enumerate(cands)])
    assert float((scores - want).abs().max()) <= 1e-3 * max(1.0, float(want.abs().max()))
    acc2, _, none = eng.evaluate(ns, hidx, mask, cands, labels, acc=acc)
    assert acc2 is acc and none is None and acc.cpu().tolist()[:2] == [6.0, 4.0]
    with pytest.raises(ValueError, match="outside the 41 rows"):
        eng.evaluate(ns, hidx, mask, [np.array([41, 0])] + cands[1:], [np.array([1, 0])] + labels[1:])
