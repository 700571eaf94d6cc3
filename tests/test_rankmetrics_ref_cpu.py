"""CPU: the float64 reference of the device rank metrics (tests/rankmetrics_ref.py) is itself right - against metrics.py, the
functions run.test calls -, and the host pieces of the feature: pack_impressions, the new flags and what check_args refuses."""
import types

import numpy as np
import pytest

import metrics
import rankmetrics_ref as R


def _host(y, s):
    return np.array([metrics.roc_auc_score(y, s), metrics.mrr_score(y, s), metrics.ndcg_score(y, s, 5), metrics.ndcg_score(y, s, 10)])


def test_reference_equals_metrics_py_without_ties():
    rng = np.random.default_rng(0)
    n = 0
    for C in list(range(2, 40)) + [63, 64, 65, 150, 299]:
        for _ in range(4):
            s = rng.permutation(C).astype(np.float32) * 0.37 - 3.0            # distinct scores
            y = np.zeros(C, np.int64)
            y[rng.permutation(C)[:rng.integers(1, C)]] = 1
            ok, got = R.impression_metrics(s, y)
            assert ok
            np.testing.assert_allclose(got, _host(y, s), rtol=0, atol=1e-12)
            n += 1
    assert n > 150


def test_reference_auc_equals_metrics_py_with_ties():
    rng = np.random.default_rng(1)
    for C in (2, 3, 7, 20, 64, 130):
        for _ in range(6):
            s = rng.integers(-2, 3, size=C).astype(np.float32)                # ties everywhere
            y = np.zeros(C, np.int64)
            y[rng.permutation(C)[:rng.integers(1, C)]] = 1
            ok, got = R.impression_metrics(s, y)
            assert ok and abs(got[0] - metrics.roc_auc_score(y, s)) <= 1e-12


def test_tie_rule_by_hand():
    """Equal scores: the later index ranks first."""
    ok, m = R.impression_metrics([1.0, 1.0, 1.0], [1, 0, 0])
    assert ok and m[1] == 1.0 / 3 and m[0] == 0.5                             # the positive comes last of the three
    ok, m = R.impression_metrics([1.0, 1.0, 1.0], [0, 0, 1])
    assert ok and m[1] == 1.0 and m[0] == 0.5 and m[2] == 1.0 and m[3] == 1.0
    # s = 2 1 1 0 with positives at 1 and 3: positions 2 (behind the later equal score) and 3
    ok, m = R.impression_metrics([2.0, 1.0, 1.0, 0.0], [0, 1, 0, 1])
    assert ok
    assert m[1] == (1.0 / 3 + 1.0 / 4) / 2
    assert m[0] == (0.5 + 0.0) / 4                                            # one tie with a negative, nothing below either
    want = (1 / np.log2(4.0) + 1 / np.log2(5.0)) / (1 / np.log2(2.0) + 1 / np.log2(3.0))
    assert abs(m[2] - want) <= 1e-15 and abs(m[3] - want) <= 1e-15
    # +0 and -0 are one score
    ok, m = R.impression_metrics(np.array([0.0, -0.0], np.float32), [1, 0])
    assert ok and m[0] == 0.5 and m[1] == 0.5
    # a small array's argsort is stable, so metrics.py shows its documented rule here
    s, y = np.array([2.0, 1.0, 1.0, 0.0], np.float32), np.array([0, 1, 0, 1])
    np.testing.assert_allclose(R.impression_metrics(s, y)[1], _host(y, s), rtol=0, atol=1e-12)


def test_skip_rule_and_totals():
    ok, m = R.impression_metrics([], [])
    assert not ok and not m.any()
    for y in ([1], [0], [1, 1, 1], [0, 0]):
        ok, m = R.impression_metrics(np.arange(len(y), dtype=np.float32), y)
        assert not ok and not m.any()
    sc = [np.array([0.3, 0.1], np.float32), np.array([0.5], np.float32), np.zeros(0, np.float32), np.array([0.1, 0.9, 0.4], np.float32)]
    ys = [np.array([1, 0]), np.array([1]), np.zeros(0, np.int64), np.array([0, 0, 1])]
    per, acc = R.launch_metrics(sc, ys)
    assert acc[0] == 4 and acc[1] == 2 and not per[1].any() and not per[2].any()
    np.testing.assert_allclose(acc[2:], per[0] + per[3], rtol=0, atol=1e-15)
    assert per[0, 0] == 1.0 and per[3, 1] == 0.5


@pytest.mark.parametrize("family", ["exact", "real"])
def test_cases_are_mostly_scored(family):
    for B in (33, 257):
        users, news, cands, labels = R.make_case(family, B, 4)
        assert R.scored_share(labels) >= 0.5
        assert [len(c) for c in cands[:10]] == list(R.SIZES)
        assert any((c == 0).any() for c in cands) and any((c == len(news) - 1).any() for c in cands)
        dup = [b for b, (c, y) in enumerate(zip(cands, labels)) if any(y[c == r].min() != y[c == r].max() for r in np.unique(c))]
        assert len(dup) >= B // 8                                             # one row, two labels
    assert R.scored_share(R.make_case(family, 1, 4)[3]) == 1.0 and R.scored_share(R.make_case(family, 3, 4)[3]) >= 0.5


def test_pack_impressions():
    from engine import pack_impressions
    cands = [np.array([5, 0, 7], np.int64), np.zeros(0, np.int64), np.array([2], np.int64)]
    labels = [np.array([0, 1, 0]), np.zeros(0, np.int64), np.array([1])]
    c, y, o = pack_impressions(cands, labels)
    assert c.dtype == y.dtype == o.dtype == np.int32
    assert o.tolist() == [0, 3, 3, 4] and c.tolist() == [5, 0, 7, 2] and y.tolist() == [0, 1, 0, 1]
    c, y, o = pack_impressions([], [])
    assert o.tolist() == [0] and c.size == 0 and y.size == 0 and c.dtype == y.dtype == o.dtype == np.int32
    with pytest.raises(ValueError, match="0 or 1"):
        pack_impressions(cands, [np.array([0, 2, 0]), labels[1], labels[2]])
    with pytest.raises(ValueError, match="index -1"):
        pack_impressions([np.array([5, -1, 7]), cands[1], cands[2]], labels)
    with pytest.raises(ValueError, match="labels"):
        pack_impressions(cands, [np.array([0, 1]), labels[1], labels[2]])
    with pytest.raises(ValueError):
        pack_impressions(cands, labels[:2])


def test_flags_and_check_args_refusals():
    import parameters
    a = parameters.build_parser().parse_args([])
    assert a.device_metrics is False and a.valid_data_dir is None and a.valid_steps == 0 and a.valid_filename_pat == "behaviors_*.tsv"
    parameters.check_args(a)
    parameters.check_args(types.SimpleNamespace())                            # a plain namespace without the new flags
    ok = parameters.build_parser().parse_args("--valid_data_dir d --valid_steps 6 --grad_accum_steps 3".split())
    parameters.check_args(ok)
    with pytest.raises(ValueError, match="needs --valid_data_dir"):
        parameters.check_args(parameters.build_parser().parse_args("--valid_steps 4".split()))
    with pytest.raises(ValueError, match="no multiple of --grad_accum_steps"):
        parameters.check_args(parameters.build_parser().parse_args("--valid_data_dir d --valid_steps 4 --grad_accum_steps 3".split()))
    with pytest.raises(ValueError):
        parameters.check_args(types.SimpleNamespace(valid_data_dir="d", valid_steps=-2))
    import engine as E
    import run
    assert callable(E.Engine.rank_metrics) and callable(E.Engine.evaluate) and callable(run._impression_loop)
