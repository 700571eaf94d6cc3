"""GPU: tnr_rank_metrics (csrc/evaluate.hip) through the C ABI against the float64 reference of tests/rankmetrics_ref.py.

Every call has sentinels behind `scores`, `per` and `acc`, NaN in the padding of the strided inputs (u_rs, n_rs > D) and in news
rows >= Nn.  A launch mixes impressions of 0, 1, 2, 63, 64, 65, 255, 256, 257 and 1000 candidates with 0, 1, 2, C - 1 and C
positives (rankmetrics_ref.make_case).  `exact` family: scores equal the reference's, `per` and `acc` are within 1e-12 per
impression of it (a few double roundings on values <= 1, the bound tests/test_n2_gpu.py holds run.test's sums to).  `real`:
scores within topk_ref.bound of float64, `per` within 1e-12 of the reference evaluated on the kernel's OWN scores."""
import functools

import numpy as np
import pytest
import torch

import rankmetrics_ref as R
import tnr_hip as T
import topk_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT_F, SENT_D = 1234.5, -4321.25
TOL = 1e-12


@functools.lru_cache(maxsize=None)
def _case(family, B, D):
    return R.make_case(family, B, D)


@functools.lru_cache(maxsize=None)
def _exact_ref(B, D):
    users, news, cands, labels = _case("exact", B, D)
    s = R.scores64(users, news, cands)
    return s, R.launch_metrics(s, labels)


def _strided(a, pad, extra_rows=0, misalign=False):
    """device (rows + extra_rows, cols + pad) fp32 view, NaN everywhere outside a's values; misalign: its base is 4 bytes
    behind a 16-byte boundary -> (tensor, row stride)."""
    rows, cols = a.shape
    ld = cols + pad
    flat = torch.full(((rows + extra_rows) * ld + 1,), float("nan"), dtype=torch.float32, device=DEV)
    t = flat[1 if misalign else 0:][:(rows + extra_rows) * ld].view(rows + extra_rows, ld)
    if rows:
        t[:rows, :cols] = torch.from_numpy(a).to(DEV)
    assert (t.data_ptr() % 16 != 0) == misalign
    return t, ld


def call_raw(users, news, cands, labels, u_pad=4, n_pad=8, misalign=False, with_per=True, acc_init=None, accumulate=0, D=None,
             B=None, null=()):
    """-> (rc, scores [per impression], per (B, 4) or None, acc (6,)) as numpy; asserts every sentinel."""
    from engine import pack_impressions
    nB = users.shape[0]
    ut, u_rs = _strided(users, u_pad, extra_rows=1, misalign=misalign)
    nt, n_rs = _strided(news, n_pad, extra_rows=3, misalign=misalign)
    c, y, o = pack_impressions(cands, labels)
    tot = int(o[-1])
    ct, yt, ot = (torch.from_numpy(np.concatenate([x, np.full(4, 10 ** 6, np.int32)])).to(DEV) for x in (c, y, o))
    sc = torch.full((tot + 32,), SENT_F, dtype=torch.float32, device=DEV)
    per = torch.full((nB * 4 + 8,), SENT_D, dtype=torch.float64, device=DEV)
    acc = torch.full((6 + 4,), SENT_D, dtype=torch.float64, device=DEV)
    if acc_init is not None:
        acc[:6] = torch.from_numpy(np.asarray(acc_init, np.float64)).to(DEV)
    before = acc.clone()
    ptr = lambda name, t: None if name in null else t.data_ptr()
    rc = T.lib().tnr_rank_metrics(ptr("users", ut), u_rs, nB if B is None else B, ptr("news", nt), n_rs, news.shape[0],
                                  users.shape[1] if D is None else D, ptr("offs", ot), ptr("cand", ct), ptr("label", yt),
                                  ptr("scores", sc), per.data_ptr() if with_per else None, ptr("acc", acc), accumulate, T.stream())
    torch.cuda.synchronize()
    assert (sc[tot:] == SENT_F).all() and (per[nB * 4:] == SENT_D).all() and (acc[6:] == SENT_D).all(), "wrote behind an output"
    if rc != 0:
        assert (sc == SENT_F).all() and (per == SENT_D).all() and torch.equal(acc, before), "a refused call wrote something"
        return rc, None, None, None
    if not with_per:
        assert (per == SENT_D).all()
    s = sc[:tot].cpu().numpy()
    return rc, [s[o[b]:o[b + 1]] for b in range(nB)], per[:nB * 4].view(nB, 4).cpu().numpy() if with_per else None, acc[:6].cpu().numpy()


def call(*a, **kw):
    rc, s, per, acc = call_raw(*a, **kw)
    assert rc == 0, T.lib().tnr_last_error().decode()
    return s, per, acc


def _bits(x):
    return np.ascontiguousarray(x).view(np.int32 if x.dtype == np.float32 else np.int64)


# every B of {0, 1, 3, 33, 257} and every D of {1, 4, 64, 100, 256, 260}; the candidate and positive counts are mixed inside
EXACT = [(0, 64), (1, 1), (1, 260), (3, 4), (3, 100), (33, 1), (33, 64), (33, 260), (257, 4), (257, 100), (257, 256)]


@pytest.mark.parametrize("B,D", EXACT)
def test_exact_family_equals_reference(B, D):
    users, news, cands, labels = _case("exact", B, D)
    rs, (rper, racc) = _exact_ref(B, D)
    if B >= 3:
        assert R.scored_share(labels) >= 0.5
    s, per, acc = call(users, news, cands, labels)
    for b in range(B):
        assert np.array_equal(s[b].astype(np.float64), rs[b]), b
    assert not np.isnan(per).any()
    err = np.abs(per - rper).max() if B else 0.0
    print("\n[rank metrics exact B %d D %d] per max |err| %.2e, acc |err| %s" % (B, D, err, np.abs(acc - racc)))
    assert err <= TOL
    assert acc[0] == B and acc[1] == racc[1]
    assert (np.abs(acc[2:] - racc[2:]) <= TOL * max(B, 1)).all()
    skipped = np.array([not 0 < int(y.sum()) < len(y) for y in labels], bool)
    assert (per[skipped] == 0).all()                                             # skipped: all four exactly 0


@pytest.mark.parametrize("B,D,misalign", [(33, 64, False), (3, 260, False), (257, 100, False), (33, 256, True)])
def test_real_family(B, D, misalign):
    users, news, cands, labels = _case("real", B, D)
    assert R.scored_share(labels) >= 0.5
    s, per, acc = call(users, news, cands, labels, u_pad=3 if misalign else 4, n_pad=1 if misalign else 8, misalign=misalign)
    s64 = R.scores64(users, news, cands)
    for b in range(B):
        if len(cands[b]):
            bd = topk_ref.bound(users[b:b + 1], news[cands[b]])[0]
            assert (np.abs(s[b].astype(np.float64) - s64[b]) <= bd).all(), b
    rper, racc = R.launch_metrics(s, labels)                                     # on the kernel's own scores
    assert np.abs(per - rper).max() <= TOL
    assert acc[0] == B and acc[1] == racc[1] and (np.abs(acc[2:] - racc[2:]) <= TOL * B).all()


def test_score_bits_equal_topk_scores():
    """129 news, every one a candidate of every user: tnr_topk_scores' 128 best carry the same score bits."""
    Nu, Nn, D, K = 5, 129, 64, 128
    users, news = topk_ref.make_inputs("real", Nu, Nn, D, seed=5)
    cands = [np.arange(Nn, dtype=np.int64)[::-1].copy() if u % 2 else np.arange(Nn, dtype=np.int64) for u in range(Nu)]
    labels = [np.arange(Nn) % 3 == 0 for _ in range(Nu)]
    s, _, _ = call(users, news, cands, [y.astype(np.int64) for y in labels])
    ut, nt = torch.from_numpy(users).to(DEV), torch.from_numpy(news).to(DEV)
    idx = torch.empty((Nu, K), dtype=torch.int32, device=DEV)
    sc = torch.empty((Nu, K), dtype=torch.float32, device=DEV)
    nb = int(T.query("tnr_topk_workspace", Nu, Nn, K, 0))
    work = torch.empty((max(nb, 8),), dtype=torch.uint8, device=DEV)
    T.call("tnr_topk_scores", ut, D, Nu, nt, D, Nn, 0, D, None, 0, 0, K, idx, sc, 0, work, nb)
    idx, sc = idx.cpu().numpy(), sc.cpu().numpy()
    assert (idx >= 0).all()
    for u in range(Nu):
        mine = np.empty(Nn, np.float32)
        mine[cands[u]] = s[u]
        assert np.array_equal(_bits(mine[idx[u]]), _bits(sc[u])), u


def test_an_impression_does_not_depend_on_its_place_or_the_strides():
    """Impressions of a 33-impression launch, alone in another order in a launch with odd strides and a misaligned base (scalar
    loads): the same score bits and the same `per` bits."""
    users, news, cands, labels = _case("real", 33, 100)
    s, per, _ = call(users, news, cands, labels)
    pick = [12, 0, 5, 32, 2, 8]
    s2, per2, acc2 = call(np.ascontiguousarray(users[pick]), news, [cands[b] for b in pick], [labels[b] for b in pick], u_pad=1,
                          n_pad=3, misalign=True)
    for a, b in enumerate(pick):
        assert np.array_equal(_bits(s2[a]), _bits(s[b])) and np.array_equal(_bits(per2[a]), _bits(per[b])), b
    assert acc2[0] == len(pick)


@pytest.mark.parametrize("family,B,D", [("real", 257, 100), ("exact", 33, 64)])
def test_two_runs_and_the_form_without_per_give_the_same_bits(family, B, D):
    users, news, cands, labels = _case(family, B, D)
    s, per, acc = call(users, news, cands, labels)
    s2, per2, acc2 = call(users, news, cands, labels)
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(s, s2))
    assert np.array_equal(_bits(per), _bits(per2)) and np.array_equal(_bits(acc), _bits(acc2))
    s3, per3, acc3 = call(users, news, cands, labels, with_per=False)
    assert per3 is None and all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(s, s3))
    assert np.array_equal(_bits(acc), _bits(acc3))


def test_accumulate_over_two_launches():
    users, news, cands, labels = _case("real", 33, 64)
    _, _, whole = call(users, news, cands, labels)
    _, _, first = call(users[:20], news, cands[:20], labels[:20])
    _, _, both = call(users[20:], news, cands[20:], labels[20:], acc_init=first, accumulate=1)
    assert both[0] == 33 and both[1] == whole[1]
    assert (np.abs(both - whole) <= TOL * 33).all()
    _, _, over = call(users[20:], news, cands[20:], labels[20:], acc_init=first, accumulate=0)
    assert over[0] == 13
    # B = 0: a no-op that zeroes acc, or leaves it
    _, _, z = call(users[:0], news, [], [], acc_init=first, accumulate=0)
    assert not z.any()
    _, _, k = call(users[:0], news, [], [], acc_init=first, accumulate=1)
    assert np.array_equal(_bits(k), _bits(first))


@pytest.mark.parametrize("what", ["D=0", "D=1025", "B=-1", "null news", "null users", "null offs", "null cand", "null label",
                                  "null scores", "null acc", "short stride"])
def test_refusals_write_nothing(what):
    users, news, cands, labels = _case("exact", 3, 4)
    kw = {}
    if what.startswith("D="):
        kw["D"] = int(what[2:])
    elif what.startswith("B="):
        kw["B"] = int(what[2:])
    elif what.startswith("null "):
        kw["null"] = (what[5:],)
    else:
        kw["D"], kw["u_pad"], kw["n_pad"] = 16, 4, 8                             # D above both strides
    rc, _, _, _ = call_raw(users, news, cands, labels, **kw)
    assert rc != 0 and b"tnr_rank_metrics" in T.lib().tnr_last_error()
