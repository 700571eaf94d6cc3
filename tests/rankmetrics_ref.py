"""float64 reference of tnr_rank_metrics (include/tnr_hip.h), computed from GIVEN scores, and the impressions the tests feed it.

The contract: an impression with P positives and Q = C - P negatives is skipped (all four values 0, counted as seen only) when
P = 0 or Q = 0.  The position of a positive i is r_i = #{j : s_j > s_i} + #{j > i : s_j == s_i} - among equal scores the later
index ranks first, what metrics._by_score documents.  Then
    AUC    = sum over positives of (#negatives s_j < s_i + 0.5 #negatives s_j == s_i) / (P Q)
    MRR    = (sum over positives of 1 / (r_i + 1)) / P
    nDCG@k = (sum over positives with r_i < k of 1 / log2(r_i + 2)) / (sum over t < min(P, k) of 1 / log2(t + 2)).

Two input families (tests/topk_ref.py's).  `exact`: operands are the integers -3 .. 3, so every score is an exact fp32 number
in any summation order and ties are everywhere: the kernel must reproduce the reference computed from the float64 scores.
`real`: standard-normal operands; the kernel's fp32 scores are within topk_ref.bound of float64, and its metrics are judged on
its OWN scores.  make_case builds impressions of which at least half are scored (P > 0 and Q > 0) once it has ten of them -
scored_share says how many, and the tests assert it, so that a skip bug cannot hide a metric bug."""
import numpy as np

# candidates per impression and positives per impression, each taken in turn; the two cycles (10 and 8 long) meet in every
# combination after 40 impressions.  Sizes 0 and 1 can never be scored; of the others the patterns "0" and "C" are not: 60 % are.
SIZES = (65, 2, 257, 0, 64, 1000, 1, 63, 255, 256)
POSITIVES = ("1", "C-1", "2", "0", "1", "C", "2", "C-1")


def impression_metrics(scores, labels):
    """-> (scored, float64 [AUC, MRR, nDCG@5, nDCG@10]) of one impression under the contract above."""
    s = np.asarray(scores, np.float64)
    y = np.asarray(labels)
    C = len(y)
    P = int((y != 0).sum())
    Q = C - P
    if P == 0 or Q == 0:
        return False, np.zeros(4)
    neg = y == 0
    idx = np.arange(C)
    auc = mrr = d5 = d10 = 0.0
    for i in np.nonzero(y != 0)[0]:
        r = int((s > s[i]).sum() + ((s == s[i]) & (idx > i)).sum())
        auc += float((neg & (s < s[i])).sum()) + 0.5 * float((neg & (s == s[i])).sum())
        mrr += 1.0 / (r + 1)
        if r < 5:
            d5 += 1.0 / np.log2(r + 2.0)
        if r < 10:
            d10 += 1.0 / np.log2(r + 2.0)
    ideal = lambda k: sum(1.0 / np.log2(t + 2.0) for t in range(min(P, k)))
    return True, np.array([auc / (float(P) * float(Q)), mrr / P, d5 / ideal(5), d10 / ideal(10)])


def launch_metrics(score_list, label_list):
    """-> (per (B, 4) float64, acc (6,) float64 = {seen, scored, the four sums}) of a launch."""
    B = len(score_list)
    per = np.zeros((B, 4))
    scored = 0
    for b, (s, y) in enumerate(zip(score_list, label_list)):
        ok, per[b] = impression_metrics(s, y)
        scored += ok
    return per, np.concatenate([[float(B), float(scored)], per.sum(0)])


def scored_share(label_list):
    n = sum(1 for y in label_list if 0 < int((np.asarray(y) != 0).sum()) < len(y))
    return n / max(len(label_list), 1)


def make_case(family, B, D, Nn=300, seed=0):
    """-> users (B, D) fp32, news (Nn, D) fp32, cands [int64 arrays], labels [int64 arrays].  Sizes and positive counts follow
    SIZES / POSITIVES in turn; candidate rows are random, with row 0 and row Nn - 1 forced into every second impression that
    has room, and in every third scored impression one positive and one negative are the SAME row (equal scores, unlike labels)."""
    rng = np.random.default_rng(seed + 1000 * B + D)
    if family == "exact":
        users = rng.integers(-3, 4, size=(B, D)).astype(np.float32)
        news = rng.integers(-3, 4, size=(Nn, D)).astype(np.float32)
    else:
        assert family == "real"
        users = rng.standard_normal((B, D)).astype(np.float32)
        news = rng.standard_normal((Nn, D)).astype(np.float32)
    cands, labels = [], []
    for b in range(B):
        C = SIZES[b % len(SIZES)]
        P = {"0": 0, "1": 1, "2": 2, "C-1": C - 1, "C": C}[POSITIVES[b % len(POSITIVES)]]
        P = min(max(P, 0), C)
        c = rng.integers(0, Nn, size=C)
        y = np.zeros(C, np.int64)
        y[rng.permutation(C)[:P]] = 1
        if C >= 2 and b % 2 == 0:
            c[rng.integers(0, C)] = 0
            c[(np.nonzero(c == 0)[0][0] + 1) % C] = Nn - 1
        if 0 < P < C and b % 3 == 0:
            c[np.nonzero(y == 1)[0][0]] = c[np.nonzero(y == 0)[0][0]]
        cands.append(c.astype(np.int64))
        labels.append(y)
    return users, news, cands, labels


def scores64(users, news, cands):
    """per impression, the float64 scores of its candidates"""
    u64, n64 = np.asarray(users, np.float64), np.asarray(news, np.float64)
    return [n64[c] @ u64[b] for b, c in enumerate(cands)]
