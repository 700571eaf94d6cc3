"""GPU: tnr_topk_scores (csrc/retrieve.hip) through the C ABI against the float64 reference of tests/topk_ref.py.

Every call has sentinels behind both outputs and behind the workspace's stated size, NaN in the padding of the strided inputs
(u_rs, n_rs > D) and in news rows >= Nn.  The `exact` family (integer operands, ties everywhere) must equal the reference
position by position; the `real` family is judged by check_result (derived fp32 bound)."""
import functools

import numpy as np
import pytest
import torch

import tnr_hip as T
import topk_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT_I, SENT_F, SENT_B = -77, 1234.5, 0xA5


@functools.lru_cache(maxsize=None)
def _inputs(family, Nu, Nn, D, seed=0):
    return R.make_inputs(family, Nu, Nn, D, seed)


@functools.lru_cache(maxsize=None)
def _ref(family, Nu, Nn, D, K, first_row=1):
    u, n = _inputs(family, Nu, Nn, D)
    return R.topk_ref(u, n, None, first_row, K)


def _strided(a, pad, extra_rows=0):
    """device (rows + extra_rows, cols + pad) fp32, NaN everywhere outside a's values -> (tensor, row stride)."""
    rows, cols = a.shape
    t = torch.full((rows + extra_rows, cols + pad), float("nan"), dtype=torch.float32, device=DEV)
    if rows:
        t[:rows, :cols] = torch.from_numpy(a).to(DEV)
    return t, cols + pad


def call_raw(users, news, excl, first_row, K, splits, u_pad=4, n_pad=8, D=None, E=None, work_short=0, news_null=False):
    """-> (rc, idx (Nu, K), score (Nu, K)) as numpy; asserts every sentinel."""
    Nu, Nn = users.shape[0], news.shape[0]
    ut, u_rs = _strided(users, u_pad)
    nt, n_rs = _strided(news, n_pad, extra_rows=3)
    D = users.shape[1] if D is None else D
    et, e_rs, E_ = None, 0, 0
    if excl is not None:
        et = torch.from_numpy(np.ascontiguousarray(excl, dtype=np.int32)).to(DEV)
        e_rs, E_ = et.shape[1], et.shape[1]
    E_ = E_ if E is None else E
    oi = torch.full((Nu * K + 32,), SENT_I, dtype=torch.int32, device=DEV)
    os_ = torch.full((Nu * K + 32,), SENT_F, dtype=torch.float32, device=DEV)
    wb = int(T.query("tnr_topk_workspace", Nu, Nn, min(max(K, 1), 128), splits))
    work = torch.full((wb + 64,), SENT_B, dtype=torch.uint8, device=DEV)
    rc = T.lib().tnr_topk_scores(ut.data_ptr(), u_rs, Nu, None if news_null else nt.data_ptr(), n_rs, Nn, first_row, D,
                                 None if et is None else et.data_ptr(), e_rs, E_, K, oi.data_ptr(), os_.data_ptr(), splits,
                                 work.data_ptr(), wb - work_short, T.stream())
    torch.cuda.synchronize()
    kk = max(K, 0)
    assert (oi[Nu * kk:] == SENT_I).all() and (os_[Nu * kk:] == SENT_F).all(), "wrote behind an output"
    assert (work[wb:] == SENT_B).all(), "wrote behind the workspace's stated size"
    if rc != 0:
        assert (oi == SENT_I).all() and (os_ == SENT_F).all() and (work == SENT_B).all(), "a refused call wrote something"
        return rc, None, None
    return rc, oi[:Nu * K].view(Nu, K).cpu().numpy(), os_[:Nu * K].view(Nu, K).cpu().numpy()


def call(users, news, excl, first_row, K, splits, **kw):
    rc, idx, sc = call_raw(users, news, excl, first_row, K, splits, **kw)
    assert rc == 0, T.lib().tnr_last_error().decode()
    return idx, sc


# a covering subset of Nu {1, 33, 65, 129} x Nn {1, K-1, K, K+1, 127, 129, 1000, 4097} x D {4, 64, 100, 256, 260} x K {1, 10, 64, 65, 128}:
# every value of every axis, K around Nn, more than one user tile, more than one news tile, D behind a 32-chunk, 3-wave (K > 96)
# and 4-wave workgroups
EXACT = [
    (1, 1, 4, 1), (1, 0, 4, 1), (1, 2, 64, 1), (33, 9, 100, 10), (33, 10, 4, 10), (65, 11, 64, 10), (1, 127, 256, 64),
    (33, 63, 260, 64), (65, 64, 100, 64), (129, 65, 4, 64), (33, 64, 64, 65), (65, 65, 256, 65), (129, 66, 260, 65),
    (1, 127, 100, 128), (33, 128, 64, 128), (65, 129, 4, 128), (129, 129, 256, 128), (129, 1000, 64, 10), (65, 1000, 260, 128),
    (129, 4097, 4, 65), (33, 4097, 256, 1), (129, 4097, 100, 128), (1, 4097, 260, 10), (65, 127, 64, 1),
]


@pytest.mark.parametrize("Nu,Nn,D,K", EXACT)
def test_exact_family_equals_reference(Nu, Nn, D, K):
    users, news = _inputs("exact", Nu, Nn, D)
    ridx, rsc = _ref("exact", Nu, Nn, D, K)
    idx, sc = call(users, news, None, 1, K, 0)
    assert np.array_equal(idx, ridx), "first differing user %d" % np.nonzero((idx != ridx).any(1))[0][0]
    assert np.array_equal(sc.astype(np.float64), rsc)


@pytest.mark.parametrize("Nu,Nn,D,K", [(129, 4097, 64, 128), (65, 1000, 100, 10), (33, 4097, 256, 64)])
def test_real_family_is_a_valid_answer(Nu, Nn, D, K):
    users, news = _inputs("real", Nu, Nn, D)
    idx, sc = call(users, news, None, 1, K, 0)
    R.check_result(users, news, None, 1, K, idx, sc)


@pytest.mark.parametrize("family,Nu,Nn,D,K", [("real", 129, 4097, 64, 128), ("exact", 65, 1000, 100, 10), ("real", 33, 4097, 256, 64)])
def test_every_split_and_every_run_gives_the_same_bits(family, Nu, Nn, D, K):
    users, news = _inputs(family, Nu, Nn, D)
    rng = np.random.default_rng(3)
    excl = rng.integers(0, Nn, size=(Nu, 7))
    base = call(users, news, excl, 1, K, 1)
    for splits in (2, 7, 0, 1, 1000):
        got = call(users, news, excl, 1, K, splits)
        assert np.array_equal(got[0], base[0]) and np.array_equal(got[1].view(np.int32), base[1].view(np.int32)), splits
    assert T.query("tnr_topk_workspace", Nu, Nn, K, 7) > T.query("tnr_topk_workspace", Nu, Nn, K, 2) > 0


def test_a_users_scores_do_not_depend_on_its_place_in_the_launch():
    """User rows 5 and 100 of a 129-user launch, alone at positions 1 and 0 of a 3-user launch with another stride, alignment
    (scalar loads) and split: the same indices and the same score bits."""
    users, news = _inputs("real", 129, 4097, 100)
    K = 64
    idx, sc = call(users, news, None, 1, K, 0)
    sub = np.ascontiguousarray(users[[100, 5, 77]])
    idx2, sc2 = call(sub, news, None, 1, K, 3, u_pad=1, n_pad=3)
    for a, b in ((0, 100), (1, 5), (2, 77)):
        assert np.array_equal(idx2[a], idx[b]) and np.array_equal(sc2[a].view(np.int32), sc[b].view(np.int32))


@pytest.mark.parametrize("E", [0, 1, 50])
@pytest.mark.parametrize("first_row", [0, 1])
def test_exclusions(E, first_row):
    Nu, Nn, D, K = 65, 1000, 64, 10
    users, news = _inputs("exact", Nu, Nn, D)
    rng = np.random.default_rng(E)
    excl = None
    if E:
        best = R.topk_ref(users, news, None, first_row, K)[0]
        excl = rng.integers(-5, Nn + 5, size=(Nu, E))                 # out-of-range ids on both sides
        excl[:, 0] = best[:, 0]                                        # the best row itself
        if E > 4:
            excl[:, 1:4] = best[:, [2, 2, 5]]                          # duplicates
            excl[:, 4] = 0                                             # the padding id
    ridx, rsc = R.topk_ref(users, news, excl, first_row, K)
    idx, sc = call(users, news, excl, first_row, K, 2)
    assert np.array_equal(idx, ridx) and np.array_equal(sc.astype(np.float64), rsc)
    R.check_result(users, news, excl, first_row, K, idx, sc)


def test_fewer_than_k_eligible_rows_and_nan_rows():
    Nu, Nn, D, K = 33, 129, 64, 65
    users, news = (a.copy() for a in _inputs("real", Nu, Nn, D))
    news[17, :] = np.nan                                               # an all-NaN news row
    users[4, :] = np.nan                                               # a NaN user: nothing is eligible
    excl = np.tile(np.arange(1, 101), (Nu, 1))                         # rows 1..100 out: 28 of 128 left (27 where row 17 is NaN's)
    idx, sc = call(users, news, excl, 1, K, 2)
    R.check_result(users, news, excl, 1, K, idx, sc)
    assert (idx[4] == -1).all() and np.isneginf(sc[4]).all()
    assert ((idx >= 0).sum(1)[np.arange(Nu) != 4] == 28).all() and not (idx == 17).any()
    idx, sc = call(users, news, None, 0, K, 1)
    R.check_result(users, news, None, 0, K, idx, sc)
    assert not (idx == 17).any() and (idx[4] == -1).all()


@pytest.mark.parametrize("what", ["K=0", "K=129", "D=6", "D=1028", "E=513", "null news", "short workspace"])
def test_refusals_launch_nothing(what):
    users, news = _inputs("exact", 33, 1000, 64)
    excl = np.zeros((33, 8), np.int32)
    kw, K = {}, 10
    if what.startswith("K="):
        K = int(what[2:])
    elif what.startswith("D="):
        kw["D"] = int(what[2:])
    elif what == "E=513":
        kw["E"] = 513
    elif what == "null news":
        kw["news_null"] = True
    else:
        kw["work_short"] = 1
    rc, _, _ = call_raw(users, news, excl, 1, K, 2, **kw)
    assert rc != 0 and len(T.lib().tnr_last_error()) > 0 and b"tnr_topk_scores" in T.lib().tnr_last_error()
