"""float64 reference of tnr_topk_scores (include/tnr_hip.h) and the judge of its results.

The contract: s(u, n) = sum_k users[u, k] * news[n, k]; row n is eligible for user u when first_row <= n < Nn, n is not in
excl[u] and s(u, n) is not NaN; a is before b iff s_a > s_b, or s_a == s_b and n_a < n_b; the result is the first K eligible
rows, then idx -1 / score -inf.

Two input families.  `exact`: operands are the integers -3 .. 3, so every partial sum is an exact fp32 number in any order
(|s| <= 9 D) and the kernel must EQUAL topk_ref position by position, ties included.  `real`: standard-normal fp32 operands;
the kernel's fp32 scores differ from float64 by at most bound(u, n) = gamma_D * sum_k |u_k n_k| with
gamma_D = D 2^-24 / (1 - D 2^-24), the textbook bound of a length-D fp32 fma chain (derived, not measured), so neighbours
closer than that may swap and the result is judged by check_result, which leaves nothing out."""
import numpy as np


def make_inputs(family, Nu, Nn, D, seed=0):
    rng = np.random.default_rng(seed)
    if family == "exact":
        return (rng.integers(-3, 4, size=(Nu, D)).astype(np.float32), rng.integers(-3, 4, size=(Nn, D)).astype(np.float32))
    assert family == "real"
    return rng.standard_normal((Nu, D)).astype(np.float32), rng.standard_normal((Nn, D)).astype(np.float32)


def scores64(users, news):
    with np.errstate(invalid="ignore"):
        return np.asarray(users, np.float64) @ np.asarray(news, np.float64).T


def bound(users, news):
    """(Nu, Nn) worst-case |fp32 chain - float64| of each score."""
    D = users.shape[1]
    g = D * 2.0 ** -24 / (1.0 - D * 2.0 ** -24)
    with np.errstate(invalid="ignore"):
        return g * (np.abs(np.asarray(users, np.float64)) @ np.abs(np.asarray(news, np.float64)).T)


def eligible(s, excl, first_row):
    """(Nu, Nn) bool.  excl: None or an int (Nu, E) array (entries outside [first_row, Nn) never match, duplicates allowed)."""
    Nu, Nn = s.shape
    ok = ~np.isnan(s)
    ok[:, :min(max(first_row, 0), Nn)] = False
    if excl is not None:
        excl = np.asarray(excl)
        for u in range(Nu):
            e = excl[u]
            e = e[(e >= 0) & (e < Nn)]
            ok[u, e] = False
    return ok


def topk_ref(users, news, excl, first_row, K):
    """-> idx int32 (Nu, K), score float64 (Nu, K): stable argsort of -score (ties to the lower index), -1 / -inf fill."""
    s = scores64(users, news)
    ok = eligible(s, excl, first_row)
    Nu = s.shape[0]
    idx = np.full((Nu, K), -1, np.int32)
    sc = np.full((Nu, K), -np.inf, np.float64)
    for u in range(Nu):
        rows = np.nonzero(ok[u])[0]
        order = rows[np.argsort(-s[u, rows], kind="stable")][:K]
        idx[u, :len(order)] = order
        sc[u, :len(order)] = s[u, order]
    return idx, sc


def check_result(users, news, excl, first_row, K, idx, score):
    """Assert that (idx, score) is a valid answer of the contract for fp32 scores within bound() of float64."""
    idx, score = np.asarray(idx), np.asarray(score)
    s = scores64(users, news)
    bd = bound(users, news)
    ok = eligible(s, excl, first_row)
    Nu, Nn = s.shape
    assert idx.shape == (Nu, K) and score.shape == (Nu, K), (idx.shape, score.shape)
    for u in range(Nu):
        n_el = int(ok[u].sum())
        n_ret = min(K, n_el)
        got, gs = idx[u], score[u]
        # (b) the -1 slots are exactly the trailing K - #eligible, with score -inf
        assert (got[:n_ret] >= 0).all() and (got[n_ret:] == -1).all(), "user %d: %d rows expected, idx %s" % (u, n_ret, got)
        assert np.isneginf(gs[n_ret:]).all(), "user %d: fill scores %s" % (u, gs[n_ret:])
        r = got[:n_ret].astype(np.int64)
        # (a) eligible rows only, none twice
        assert (r < Nn).all() and ok[u, r].all(), "user %d returns ineligible rows %s" % (u, r[~ok[u, np.minimum(r, Nn - 1)]])
        assert len(np.unique(r)) == n_ret, "user %d returns a row twice" % u
        # (c) each score within the chain's bound of float64
        err = np.abs(gs[:n_ret].astype(np.float64) - s[u, r])
        assert not np.isnan(gs[:n_ret]).any() and (err <= bd[u, r]).all(), \
            "user %d: score error %g over the bound %g" % (u, err.max(), bd[u, r][err.argmax()])
        # (d) the contract's order under the result's OWN scores
        a, b = gs[:n_ret][:-1], gs[:n_ret][1:]
        assert ((a > b) | ((a == b) & (r[:-1] < r[1:]))).all(), "user %d: list out of order" % u
        # (e) no eligible row left out could belong in front of the last one
        if n_ret:
            rest = ok[u].copy()
            rest[r] = False
            last = r[-1]
            over = s[u, rest] > s[u, last] + bd[u, rest] + bd[u, last]
            assert not over.any(), "user %d: row %d left out" % (u, np.nonzero(rest)[0][over.argmax()])
