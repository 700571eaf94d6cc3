"""float64 reference of the in-batch negatives of the target loss (include/tnr_hip.h, csrc/inbatch.hip), written straight from the
definition in plain loops, and the id fixtures the GPU tests feed.  Imports no GPU module; tests/test_inbatch_ref_cpu.py ties it to
torch autograd, to heads_ref.kd_score_loss and to a hand-worked example, and holds every fixture to the fixture condition.

A batch of B impressions has M = B C candidate slots; slot j = b' C + c' holds news id cand_ids[b', c'].  Foreign slot j is a
negative of impression b, E[b, j] = 1, iff
  1. b' != b;  2. its id is not 0;  3. no slot j' < j holds the same id;  4. the id is not among cand_ids[b, :];
  5. the id is not among hist_ids[b, :] (all U entries, whatever the mask).
target_b = -log softmax(score[b, :] U {z[b, j] = u_b . v_j : E[b, j]})[label_b],  target = mean_b target_b.

eligibility_v / words_v / loss_v / bwd_v are the same in vectorised numpy, for the fixtures at the kernels' limits (LIMITS, up to
8192 slots), where the loops take minutes; the CPU test holds them to the loops on every fixture the loops can do."""
import numpy as np

F64 = np.float64


def eligibility(hist_ids, cand_ids, stages=False):
    """-> E (B, M) uint8.  stages=True: -> [E after rule 1, after rules 1-2, 1-3, 1-4, 1-5], each (B, M)."""
    hist_ids, cand_ids = np.asarray(hist_ids), np.asarray(cand_ids)
    B, C = cand_ids.shape
    M = B * C
    flat = [int(x) for x in cand_ids.reshape(-1)]
    hist = [[int(x) for x in row] for row in hist_ids.reshape(B, -1)]
    own = [flat[b * C:(b + 1) * C] for b in range(B)]
    first = [flat[j] not in flat[:j] for j in range(M)]                 # rule 3 depends on the slot alone
    out = [np.zeros((B, M), np.uint8) for _ in range(5)]
    for b in range(B):
        for j in range(M):
            n = flat[j]
            r = [j // C != b, n != 0, first[j], n not in own[b], n not in hist[b]]
            for s in range(5):
                out[s][b, j] = all(r[:s + 1])
    return out if stages else out[4]


def words(E):
    """The mask as the kernels carry it: (B, ceil(M / 32)) uint32, bit j % 32 of word j // 32 of row b = E[b, j]."""
    E = np.asarray(E)
    B, M = E.shape
    W = (M + 31) // 32
    w = np.zeros((B, W), np.uint64)
    for b in range(B):
        for j in range(M):
            if E[b, j]:
                w[b, j // 32] |= np.uint64(1 << (j % 32))
    return w.astype(np.uint32)


def logits(users, cands):
    """z (B, M) = u_b . v_j in float64, and sum_k |u_bk v_jk| (the magnitude the fixed-order sum bound takes)."""
    u, v = np.asarray(users, F64), np.asarray(cands, F64)
    return u @ v.T, np.abs(u) @ np.abs(v).T


def loss(users, cands, score, label, E, coef):
    """-> dict(target, per (B,), dscore_add (B, C) = coef (p - onehot) / B, dz (B, M) = coef p / B on E and 0 elsewhere, z (B, M))."""
    score = np.asarray(score, F64)
    B, C = score.shape
    E = np.asarray(E).astype(bool)
    M = E.shape[1]
    u, v = np.asarray(users, F64), np.asarray(cands, F64)
    z = np.zeros((B, M), F64)
    per, dscore_add, dz = np.zeros(B, F64), np.zeros((B, C), F64), np.zeros((B, M), F64)
    for b in range(B):
        js = [j for j in range(M) if E[b, j]]
        for j in js:
            z[b, j] = float(np.dot(u[b], v[j]))
        lg = np.concatenate([score[b], z[b, js]])
        mx = lg.max()
        lse = mx + np.log(np.exp(lg - mx).sum())
        p = np.exp(lg - lse)
        y = int(label[b])
        per[b] = -(score[b, y] - lse)
        for c in range(C):
            dscore_add[b, c] = coef * (p[c] - (1.0 if c == y else 0.0)) / B
        for i, j in enumerate(js):
            dz[b, j] = coef * p[C + i] / B
    return dict(target=float(per.mean()), per=per, dscore_add=dscore_add, dz=dz, z=z)


def bwd(dz, users, cands):
    """-> duser (B, D) = sum_j dz[b, j] v_j, dcand (M, D) = sum_b dz[b, j] u_b (what is ADDED to the rows' gradients)."""
    dz, u, v = np.asarray(dz, F64), np.asarray(users, F64), np.asarray(cands, F64)
    B, M = dz.shape
    duser, dcand = np.zeros_like(u[:B]), np.zeros_like(v[:M])
    for b in range(B):
        for j in range(M):
            if dz[b, j] != 0.0:
                duser[b] += dz[b, j] * v[j]
                dcand[j] += dz[b, j] * u[b]
    return duser, dcand


# ---------------------------------------------------------------------------------------------- the same, vectorised (float64)
# The loops above are the definition; at 8192 slots they take minutes.  tests/test_inbatch_ref_cpu.py holds these to them on
# every fixture the loops can still do: the mask exactly, the loss and the gradients to 1e-12.
def eligibility_v(hist_ids, cand_ids, stages=False):
    hist_ids, cand_ids = np.asarray(hist_ids), np.asarray(cand_ids)
    B, C = cand_ids.shape
    M = B * C
    flat = cand_ids.reshape(-1)
    hist = hist_ids.reshape(B, -1)
    first = np.zeros(M, bool)
    first[np.unique(flat, return_index=True)[1]] = True                # the index of each id's first slot
    foreign = (np.arange(M) // C)[None, :] != np.arange(B)[:, None]
    own, clicked = np.zeros((B, M), bool), np.zeros((B, M), bool)
    for b in range(B):
        own[b], clicked[b] = np.isin(flat, cand_ids[b]), np.isin(flat, hist[b])
    out = [foreign]
    for rule in ((flat != 0)[None, :], first[None, :], ~own, ~clicked):
        out.append(out[-1] & rule)
    out = [s.astype(np.uint8) for s in out]
    return out if stages else out[4]


def words_v(E):
    E = np.asarray(E).astype(bool)
    B, M = E.shape
    W = (M + 31) // 32
    pad = np.zeros((B, W * 32), bool)
    pad[:, :M] = E
    by = np.packbits(pad.reshape(B, W, 4, 8), axis=-1, bitorder="little")[..., 0].astype(np.uint32)      # bytes, low first
    return by[..., 0] | (by[..., 1] << np.uint32(8)) | (by[..., 2] << np.uint32(16)) | (by[..., 3] << np.uint32(24))


def loss_v(users, cands, score, label, E, coef):
    """loss(); rows of cands that are eligible for nobody are never read (they may hold NaN).  A label outside [0, C): that
    impression's per and the target are NaN, its dscore_add is coef p / B (no candidate is the positive), as the kernel has it."""
    score = np.asarray(score, F64)
    B, C = score.shape
    E = np.asarray(E).astype(bool)
    u, v = np.asarray(users, F64)[:B], np.asarray(cands, F64)[:E.shape[1]]
    v = np.where(E.any(0)[:, None], v, 0.0)
    z = np.where(E, u @ v.T, 0.0)
    zm = np.where(E, z, -np.inf)
    mx = np.maximum(score.max(1), zm.max(1))
    lse = mx + np.log(np.exp(score - mx[:, None]).sum(1) + np.exp(zm - mx[:, None]).sum(1))
    label = np.asarray(label).astype(np.int64)
    ok = (label >= 0) & (label < C)
    onehot = (np.arange(C)[None, :] == label[:, None]).astype(F64)
    per = np.where(ok, lse - score[np.arange(B), np.where(ok, label, 0)], np.nan)
    return dict(target=float(per.mean()), per=per, dscore_add=coef * (np.exp(score - lse[:, None]) - onehot) / B,
                dz=np.where(E, coef * np.exp(zm - lse[:, None]) / B, 0.0), z=z)


def bwd_v(dz, users, cands):
    """bwd(); rows of cands whose dz column is all zero are never read."""
    dz, u, v = np.asarray(dz, F64), np.asarray(users, F64), np.asarray(cands, F64)
    B, M = dz.shape
    v = np.where((dz != 0.0).any(0)[:, None], v[:M], 0.0)
    return dz @ v, dz.T @ u[:B]


# ------------------------------------------------------------------------------------------------------------------ fixtures
def condition(hist_ids, cand_ids):
    """The fixture condition: each of rules 2 - 5 removes at least one slot the rules before it left, at least one foreign slot is
    eligible for at least two impressions, and at least one impression has none.  -> dict of booleans, all of which must hold."""
    s = eligibility(hist_ids, cand_ids, stages=True)
    out = {"rule %d removes a slot" % (r + 1): bool((s[r - 1] > s[r]).any()) for r in range(1, 5)}
    out["a slot eligible for two impressions"] = bool((s[4].sum(0) >= 2).any())
    out["an impression with none"] = bool((s[4].sum(1) == 0).any())
    return out


def draw_small(B, U, C, seed, n_ids=7):
    """Ids from range(n_ids), 0 (the padding news) included: at a handful of impressions they collide in every way."""
    rs = np.random.RandomState(seed)
    return rs.randint(0, n_ids, (B, U)).astype(np.int32), rs.randint(0, n_ids, (B, C)).astype(np.int32)


def draw_wide(B, U, C, seed):
    """Mostly distinct ids, for shapes with more slots than a small range can keep eligible: cand ids from a range of 4 B C with a
    few padding ids, a few repeats and a few ids another impression clicked; the LAST impression's history (U >= B C) lists every
    id of the batch, so it has no negative; impression 0 clicked a news of impression 1, and holds one of impression 2's as a
    candidate of its own."""
    M = B * C
    assert U >= M and B >= 4 and C >= 2
    rs = np.random.RandomState(seed)
    cand = (1 + rs.permutation(4 * M)[:M]).astype(np.int32).reshape(B, C)
    hist = rs.randint(4 * M + 1, 5 * M, (B, U)).astype(np.int32)        # clicked news nobody has as a candidate
    hist[:, :U // 2] = 0                                                  # left padding
    cand[1, 0] = 0                                                        # rule 2
    cand[B - 2, C - 1] = cand[1, 1]                                       # rule 3: a repeat of an earlier slot
    cand[0, 1] = cand[2, 0]                                               # rule 4 for impression 0 (and rule 3 for slot (2, 0))
    cand[3, 0] = cand[2, 1]                                               # rule 3 again; the first slot (2, 1) stays eligible
    cand[3, 1] = cand[0, 0]                                               # rule 4 for impression 3: slot (0, 0) is its own news too
    hist[0, U - 1] = cand[1, 1]                                           # rule 5 for impression 0
    hist[B - 1, :M] = cand.reshape(-1)                                    # the last impression clicked everything
    return hist, cand


def draw_engine(B, U, C, seed, n_news=12):
    """A feed of the engine tests: rows of a news table of n_news + 1 rows (row 0 the padding news), histories left-padded with
    the padding news down to at most four clicks, so that not every news of the table is clicked by everybody.
    -> (hist_idx, cand_idx, mask (B, U) float32, label (B,) int64)."""
    rs = np.random.RandomState(seed)
    hist = rs.randint(1, n_news + 1, (B, U)).astype(np.int32)
    mask = np.ones((B, U), np.float32)
    for b in range(B):
        k = U - rs.randint(0, 5)
        hist[b, :k], mask[b, :k] = 0, 0
    assert U >= n_news
    hist[1, U - n_news:], mask[1, U - n_news:] = 1 + rs.permutation(n_news), 1      # impression 1 clicked every news: no negative
    cand =rs.randint(0, n_news + 1, (B, C)).astype(np.int32)
    return hist, cand, mask, rs.randint(0, C, B).astype(np.int64)


# name -> (hist_ids (B, U) int32, cand_ids (B, C) int32).  The small ones: seeds picked so that the condition holds
# (test_inbatch_ref_cpu.py asserts it for every entry).
_SMALL = {"b3": (3, 3, 2, 22), "b4": (4, 3, 2, 11), "b5": (5, 3, 2, 0), "s5": (5, 3, 1, 7)}
_WIDE = {"m65": (13, 65, 5, 1), "m600": (40, 600, 15, 2)}
_ENGINE = {"e3": (3, 20, 5, 0), "e4": (4, 20, 5, 0), "e5": (5, 20, 5, 0), "e5b": (5, 20, 5, 1)}     # history_ref's U, C
_MEMO = {}


def engine_feed(name):
    """-> (hist_idx, cand_idx, mask, label) of an engine fixture, built once."""
    if name not in _MEMO:
        _MEMO[name] = draw_engine(*_ENGINE[name])
    return _MEMO[name]


def fixture(name):
    if name in _ENGINE:
        return engine_feed(name)[:2]
    if name not in _MEMO:
        _MEMO[name] = draw_small(*_SMALL[name]) if name in _SMALL else draw_wide(*_WIDE[name])
    return _MEMO[name]


FIXTURES = sorted(_SMALL) + sorted(_WIDE) + sorted(_ENGINE)


# ------------------------------------------------------------------------------------------- fixtures at the kernels' limits
# The kernels take their slots 256 at a time (ib_first_kernel: a workgroup per 256 slots, ib_elig_kernel and ib_loss_kernel: a
# round per 256 slots), ib_loss_kernel sums the exponentials of the eligible slots by RANK, 256 ranks a round, and at 8192 slots
# every LDS array of it is full.  These sit on those edges; too large for the loops above, they go through the vectorised forms.
def draw_distinct(B, U, C, seed):
    """No id twice, none 0: every impression has exactly (B - 1) C eligible slots."""
    ids = 1 + np.random.RandomState(seed).permutation(B * (U + C)).astype(np.int32)
    return ids[:B * U].reshape(B, U), ids[B * U:].reshape(B, C)


def draw_mixed(B, U, C, seed):
    """draw_small with the range growing with the batch, half as many ids as slots: about four slots in ten repeat an earlier
    one, histories and own candidates hit, 0 is drawn now and then - and most impressions keep many negatives."""
    return draw_small(B, U, C, seed, n_ids=max(7, B * C // 2))


MAX_MIXED_U = 4600


def draw_max_mixed(seed=5):
    """512 x 16 = 8192 slots, ids from range(1, 6000) (about 4470 distinct, the other slots repeats), and
      - slots 32..63 hold ids nobody else holds: the second word of every other impression's row is all ones;
      - slots 64..95 hold the padding news: the third word of every row is all zeros, those rows are eligible for nobody;
      - impression b clicked b % 61 news of the range (rule 5), impression 7 two thousand; the rest of a history is padding;
      - the last impression clicked every news of the batch: no negative."""
    B, C, U = 512, 16, MAX_MIXED_U
    rs = np.random.RandomState(seed)
    cand = rs.randint(1, 6000, (B, C)).astype(np.int32)
    cand.reshape(-1)[32:64] = 6000 + np.arange(32)
    cand.reshape(-1)[64:96] = 0
    hist = np.zeros((B, U), np.int32)
    for b in range(B):
        k = 2000 if b == 7 else b % 61
        hist[b, U - k:] = rs.randint(1, 6000, k)
    ids = np.unique(cand)
    assert ids.size <= U
    hist[B - 1, :] = 0
    hist[B - 1, U - ids.size:] = ids
    return hist, cand


# name -> (B, C, drawer, seed, eligible slots per impression or None)
LIMITS = {"r255": (18, 15, draw_distinct, 1, 255), "r256": (17, 16, draw_distinct, 2, 256), "r257": (258, 1, draw_distinct, 3, 257),
          "s255": (51, 5, draw_mixed, 4, None), "s256": (16, 16, draw_mixed, 5, None), "s257": (257, 1, draw_mixed, 6, None),
          "s512": (32, 16, draw_mixed, 7, None), "s513": (171, 3, draw_mixed, 8, None),
          "max": (512, 16, draw_distinct, 9, 8176), "max_mixed": (512, 16, None, 5, None), "w8191": (8191, 1, draw_mixed, 10, None)}
LIMIT_SLOTS = {"r255": 270, "r256": 272, "r257": 258, "s255": 255, "s256": 256, "s257": 257, "s512": 512, "s513": 513,
               "max": 8192, "max_mixed": 8192, "w8191": 8191}
LIMIT_FIXTURES = list(LIMITS)


def limit_fixture(name, U=3):
    """-> (hist_ids (B, U), cand_ids (B, C)) of a fixture at the limits; U is free except for max_mixed, whose histories are its
    own (MAX_MIXED_U wide).  Built once per (name, U); treat as read-only."""
    if name == "max_mixed":
        U = MAX_MIXED_U
    if (name, U) not in _MEMO:
        B, C, draw, seed, _ = LIMITS[name]
        _MEMO[name, U] = draw_max_mixed(seed) if draw is None else draw(B, U, C, seed)
    return _MEMO[name, U]


def limit_eligibility(name, U=3):
    """eligibility_v of a limit fixture, computed once."""
    if ("E", name, U) not in _MEMO:
        _MEMO["E", name, U] = eligibility_v(*limit_fixture(name, U))
    return _MEMO["E", name, U]


def max_mixed_conditions(E):
    """What the max_mixed fixture is for, as booleans that must all hold."""
    w = words_v(E)
    some = (w != 0).any(1)
    return {"an impression with no eligible slot": bool((E.sum(1) == 0).any()),
            "an impression with more than 4096": bool((E.sum(1) > 4096).any()),
            "a word of all ones": bool((w == 0xFFFFFFFF).any()),
            "a word of all zeros in a row with set bits": bool(((w == 0) & some[:, None]).any()),
            "a candidate row eligible for nobody": bool((E.sum(0) == 0).any()),
            "counts vary": bool(np.unique(E.sum(1)).size > 50)}
