"""CPU: the float64 reference and judge of the top-K retrieval kernel (tests/topk_ref.py) are themselves right - topk_ref against
a brute-force sort with the contract's key, check_result accepts the reference's own answer and rejects each seeded defect -
and the feature's host surface exists: the mode, the flags, the engine methods, the workspace query."""
import functools

import numpy as np
import pytest

import topk_ref as R


def _brute(users, news, excl, first_row, K):
    s = R.scores64(users, news)
    out = []
    for u in range(s.shape[0]):
        banned = set() if excl is None else set(int(e) for e in excl[u])
        rows = [n for n in range(s.shape[1]) if n >= first_row and n not in banned and not np.isnan(s[u, n])]
        rows = sorted(rows, key=functools.cmp_to_key(
            lambda a, b: -1 if (s[u, a] > s[u, b] or (s[u, a] == s[u, b] and a < b)) else 1))[:K]
        out.append(([int(r) for r in rows] + [-1] * (K - len(rows)), [s[u, r] for r in rows] + [-np.inf] * (K - len(rows))))
    return np.array([o[0] for o in out], np.int32), np.array([o[1] for o in out])


@pytest.mark.parametrize("family", ["exact", "real"])
@pytest.mark.parametrize("Nu,Nn,D,K,first_row,E", [(3, 1, 4, 1, 1, 0), (4, 9, 4, 10, 0, 2), (5, 30, 8, 7, 1, 5), (2, 12, 4, 12, 1, 40)])
def test_reference_against_brute_force(family, Nu, Nn, D, K, first_row, E):
    users, news = R.make_inputs(family, Nu, Nn, D, seed=Nn)
    if Nn > 5:
        news[3, 0] = np.nan
    excl = np.random.default_rng(1).integers(-2, Nn + 2, size=(Nu, E)) if E else None
    idx, sc = R.topk_ref(users, news, excl, first_row, K)
    bi, bs = _brute(users, news, excl, first_row, K)
    assert np.array_equal(idx, bi) and np.array_equal(sc, bs)
    assert not (idx == 3).any() or Nn <= 5


CASES = {"exact": (5, 200, 16, 12), "real": (5, 200, 64, 12)}


def _answer(family, excl_rows=True):
    Nu, Nn, D, K = CASES[family]
    users, news = R.make_inputs(family, Nu, Nn, D, seed=2)
    news[7, :] = np.nan                                                 # a NaN-scored row
    excl = np.tile(np.array([[11, 12, 0, 500, -3]]), (Nu, 1))
    idx, sc = R.topk_ref(users, news, excl, 1, K)
    return users, news, excl, K, idx, sc.astype(np.float32)


@pytest.mark.parametrize("family", ["exact", "real"])
def test_check_result_accepts_the_reference(family):
    users, news, excl, K, idx, sc = _answer(family)
    R.check_result(users, news, excl, 1, K, idx, sc)
    # fewer eligible rows than K: trailing -1 / -inf
    few = np.tile(np.arange(1, 195), (users.shape[0], 1))
    idx2, sc2 = R.topk_ref(users, news, few, 1, K)
    assert (idx2[:, 5:] == -1).all() and (idx2[:, :5] >= 195).all()     # 195 .. 199 are left
    R.check_result(users, news, few, 1, K, idx2, sc2.astype(np.float32))


def _rejected(users, news, excl, K, idx, sc, ridx=None, rsc=None):
    """True when check_result or (exact family: ridx given) the position-wise comparison fails."""
    try:
        R.check_result(users, news, excl, 1, K, idx, sc)
    except AssertionError:
        return True
    return ridx is not None and not (np.array_equal(idx, ridx) and np.array_equal(sc, rsc))


@pytest.mark.parametrize("defect", ["tied swapped", "best dropped", "excluded present", "row 0 present", "duplicate", "missing fill",
                                    "nan row present", "score off"])
def test_seeded_defects_are_caught(defect):
    family = "exact" if defect == "tied swapped" else "real"
    users, news, excl, K, ridx, rsc = _answer(family)
    idx, sc = ridx.copy(), rsc.copy()
    s = R.scores64(users, news)
    u = 2
    if defect == "tied swapped":
        ties = [(uu, j) for uu in range(idx.shape[0]) for j in range(K - 1) if sc[uu, j] == sc[uu, j + 1]]
        assert ties, "the exact family has ties among the first K"
        uu, j = ties[0]
        idx[uu, [j, j + 1]] = idx[uu, [j + 1, j]]                       # only the position-wise comparison can see this
        try:
            R.check_result(users, news, excl, 1, K, idx, sc)
            caught_by_judge = False
        except AssertionError:
            caught_by_judge = True
        assert caught_by_judge                                          # (d): equal scores must come in ascending index
    elif defect == "best dropped":
        nxt = R.topk_ref(users, news, excl, 1, K + 1)
        idx[u], sc[u] = nxt[0][u, 1:], nxt[1][u, 1:].astype(np.float32)
    elif defect == "excluded present":
        idx[u, -1], sc[u, -1] = 11, np.float32(s[u, 11])
        order = np.argsort(-sc[u], kind="stable")
        idx[u], sc[u] = idx[u, order], sc[u, order]
    elif defect == "row 0 present":
        idx[u, -1], sc[u, -1] = 0, np.float32(s[u, 0])
        order = np.argsort(-sc[u], kind="stable")
        idx[u], sc[u] = idx[u, order], sc[u, order]
    elif defect == "duplicate":
        idx[u, 1], sc[u, 1] = idx[u, 0], sc[u, 0]
    elif defect == "missing fill":
        few = np.tile(np.arange(1, 195), (users.shape[0], 1))
        idx, sc = R.topk_ref(users, news, few, 1, K)
        idx, sc = idx.copy(), sc.astype(np.float32)
        excl = few
        idx[u, 5], sc[u, 5] = 0, -np.inf                                # a slot that should be -1
        assert _rejected(users, news, excl, K, idx, sc)
        idx[u, 5], sc[u, 5] = -1, np.float32(-1e30)                     # a fill score that is not -inf
    elif defect == "nan row present":
        idx[u, -1], sc[u, -1] = 7, np.float32(np.nan)
    else:
        j = 3
        sc[u, j] += np.float32(4.0 * R.bound(users, news)[u, idx[u, j]])
    assert _rejected(users, news, excl, K, idx, sc, ridx if family == "exact" else None, rsc)


def test_host_surface():
    import engine as E
    import parameters
    import tnr_hip as T
    from dataloader import DataLoaderRecommend, DataLoaderTest
    a = parameters.build_parser().parse_args(["--mode", "recommend"])
    assert a.mode == "recommend" and a.top_k == 10 and a.recommend_out is None and a.exclude_history is True
    b = parameters.build_parser().parse_args([])
    assert b.mode == "train" and b.top_k == 10 and b.exclude_history is True
    assert callable(E.Engine.topk) and callable(E.Engine.recommend)
    assert issubclass(DataLoaderRecommend, DataLoaderTest) and DataLoaderRecommend._process is not DataLoaderTest._process
    import run
    assert callable(run.recommend)
    # the workspace query is host arithmetic: it answers without a GPU, grows with splits, and one part needs none
    w = [T.query("tnr_topk_workspace", 4096, 51200, 100, s) for s in (1, 2, 7)]
    assert w[0] == 0 and 0 < w[1] < w[2] and w[1] == 4096 * 2 * 100 * 8
    assert T.query("tnr_topk_workspace", 32, 51200, 10, 0) > 0
    assert T.query("tnr_topk_workspace", 32, 51200, 129, 2) == 0          # a request tnr_topk_scores refuses
