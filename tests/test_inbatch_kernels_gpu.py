"""The in-batch-negatives kernels (csrc/inbatch.hip: tnr_inbatch_plan / tnr_inbatch_loss / tnr_inbatch_bwd), one by one through
tnr_hip, against the float64 reference of tests/inbatch_ref.py (tied down by tests/test_inbatch_ref_cpu.py, which also holds the id
fixtures used here to the fixture condition).  No engine.

Every output has a sentinel region behind it that must come back untouched, and every kernel runs twice and must give the same
bits (test_heads_kernels_gpu.py's Buf / twice).  Bounds (that file's): the logits z are fixed-order fp32 sums of D rounded
products, (D + 1) 2^-23 sum|u_k v_k|; per-impression losses and losses[1] FWD = 1e-4; dz and the dscore increment DSCORE = 1e-3,
duser / dcand DVEC = 1e-3, each with the floor of 1e-5 of the tensor's largest magnitude.  The plan is integers: equal.
The outputs the kernels ADD into are run twice: from zeros, where the increment itself is held to its bound, and pre-filled,
where every element must be the correctly rounded fp32 sum of the pre-filled value and that increment, bit for bit (the bound of
the increment says nothing about the rounding of an add into a larger value).

Shapes that are degenerate by design and so outside the fixture condition: B = 1 (no foreign slot), the all-distinct plan case and
the plan's sweep over the word edges; their masks are compared with inbatch_ref.eligibility() like every other.

At the kernels' limits (inbatch_ref.LIMITS: 255 / 256 / 257 eligible slots per impression, 255 ... 513 slots, 8192 slots at D = 1024,
8191 slots) the reference is the vectorised float64 form of the same file, which tests/test_inbatch_ref_cpu.py holds to the loops;
the bounds are the same functions.  Measured on one MI355X, worst error / bound over those cases: z 0.078, per-impression loss
0.021, losses[1] 0.001, dz 0.158, dscore 0.016, duser 0.056, dcand 0.021."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import inbatch_ref as R                                                        # noqa: E402
import tnr_hip as T                                                            # noqa: E402
from test_heads_kernels_gpu import (Buf, twice, rnd, dev, check, check_sum,    # noqa: E402
                                    SENT, FWD, DSCORE, DVEC)

DEV = "cuda:0"
ISENT = 0x5A5A5A5A


class IBuf:
    """Buf for 32-bit integer outputs (int32 storage; compare through bits())."""

    def __init__(self, *shape):
        n = int(np.prod(shape))
        self.raw = torch.full((n + 64,), ISENT, device=DEV, dtype=torch.int32)
        self.t = self.raw[:n].view(*shape)

    def guard_ok(self):
        return bool((self.raw[self.t.numel():] == ISENT).all())

    def bits(self):
        return self.t.cpu().numpy().view(np.uint32)


def twice_int(fn):
    a, b = fn(), fn()
    torch.cuda.synchronize()
    for n in a:
        assert a[n].guard_ok() and b[n].guard_ok(), "%s: wrote behind its buffer" % n
        assert torch.equal(a[n].t, b[n].t), "%s: two runs differ" % n
    return {n: a[n].bits() for n in a}


def run_plan(hist, cand):
    B, C = cand.shape
    U = hist.shape[1]
    W = (B * C + 31) // 32

    def fn():
        o = dict(elig=IBuf(B, W), count=IBuf(B), first=IBuf(W))
        T.call("tnr_inbatch_plan", dev(hist), dev(cand), o["elig"].t, o["count"].t, o["first"].t, B, U, C)
        return o
    return twice_int(fn)


# ------------------------------------------------------------------------------------------------ tnr_inbatch_plan
@pytest.mark.parametrize("U", [1, 3, 50])
@pytest.mark.parametrize("B,C", [(1, 5), (2, 1), (3, 2), (5, 2), (31, 1), (16, 2), (11, 3), (13, 5), (5, 16)])
def test_plan_at_the_word_edges(B, C, U):
    """B C = 5, 2, 6, 10, 31, 32, 33, 65, 80 slots: below, at and above one and two 32-bit words; ids from a range of 7 with 0."""
    hist, cand = R.draw_small(B, U, C, 100 * B + 10 * C + U)
    E = R.eligibility(hist, cand)
    got = run_plan(hist, cand)
    assert (got["elig"] == R.words(E)).all()                   # bits at and above B C are zero in the reference's words
    assert (got["count"].view(np.int32) == E.sum(1)).all()     # (first_ws is workspace: only its guard is looked at)


@pytest.mark.parametrize("name", R.FIXTURES)
def test_plan_of_the_fixtures(name):
    hist, cand = R.fixture(name)
    E = R.eligibility(hist, cand)
    got = run_plan(hist, cand)
    assert (got["elig"] == R.words(E)).all() and (got["count"].view(np.int32) == E.sum(1)).all()


def test_plan_all_distinct_ids():
    """Nothing collides: every foreign slot is eligible, count = (B - 1) C."""
    B, U, C = 7, 4, 5
    ids = 1 + np.random.RandomState(3).permutation(B * (U + C)).astype(np.int32)
    hist, cand = ids[:B * U].reshape(B, U), ids[B * U:].reshape(B, C)
    E = R.eligibility(hist, cand)
    assert (E.sum(1) == (B - 1) * C).all()
    got = run_plan(hist, cand)
    assert (got["elig"] == R.words(E)).all() and (got["count"].view(np.int32) == (B - 1) * C).all()


# ------------------------------------------------------------------------------------------------ tnr_inbatch_loss
def loss_inputs(name, D, scale, seed, nan_rows=True):
    """users scaled so that the logits have magnitude `scale`; the rows of slots that are eligible for nobody are NaN."""
    if name == "one":                                           # B = 1, C = 5: five slots, no foreign one
        hist, cand = np.zeros((1, 3), np.int32), np.arange(1, 6, dtype=np.int32).reshape(1, 5)
    else:
        hist, cand = R.fixture(name)
    B, C = cand.shape
    E = R.eligibility(hist, cand)
    users = rnd((B, D), seed, scale / np.sqrt(D))
    cands = rnd((B * C, D), seed + 1)
    if nan_rows:
        cands[E.sum(0) == 0] = np.nan
    score = rnd((B, C), seed + 2, scale)
    label = np.random.RandomState(seed).randint(0, C, B).astype(np.int64)
    return users, cands, score, label, E


def strided(x, pad):
    """x (n, D) on the device as rows of D + pad floats, the padding NaN."""
    if not pad:
        return dev(x)
    t = torch.full((x.shape[0], x.shape[1] + pad), float("nan"), device=DEV)
    t[:, :x.shape[1]] = dev(x)
    return t


def run_loss(users, cands, score, label, E, coef, pre, pad=0, want_z=True):
    B, C = score.shape
    D, M = users.shape[1], B * C
    words = dev(R.words_v(E).view(np.int32))
    u, v, s, y = strided(users, pad), strided(cands, pad), dev(score), dev(label)

    def fn():
        o = dict(dscore=Buf(B, C, fill=pre), dz=Buf(B, M), z=Buf(B, M), per=Buf(B), losses=Buf(4))
        T.call("tnr_inbatch_loss", u, D + pad, v, D + pad, s, y, words, coef, o["dscore"].t, o["dz"].t,
               o["z"].t if want_z else None, o["per"].t, o["losses"].t, B, C, D)
        return o
    return twice(fn)


LOSS_CASES = [("one", 4, 1.0, 0.2), ("one", 64, 30.0, 1.0), ("s5", 8, 1.0, 1.0), ("s5", 68, 30.0, 0.2), ("b5", 8, 1.0, 0.2),
              ("b5", 60, 30.0, 1.0), ("m65", 4, 30.0, 0.2), ("m65", 64, 1.0, 1.0), ("m65", 68, 1.0, 0.2), ("m65", 256, 30.0, 1.0),
              ("m600", 8, 1.0, 1.0), ("m600", 60, 30.0, 0.2), ("m600", 256, 1.0, 0.2), ("m600", 256, 30.0, 1.0)]


@pytest.mark.parametrize("name,D,scale,coef", LOSS_CASES)
def test_loss(name, D, scale, coef):
    """5, 5, 10, 65 and 600 slots: one slot round, a second wave, a second round of 256 slots (and a third); D below, at and above
    the 32-wide staged chunk and its multiples.  scale 30: logits of magnitude 30, where a missing max subtraction overflows."""
    users, cands, score, label, E = loss_inputs(name, D, scale, 7 * D + len(name))
    B, C = score.shape
    pre = rnd((B, C), D, 0.01)
    ref = R.loss(users, cands, score, label, E, coef)
    got = run_loss(users, cands, score, label, E, coef, np.zeros((B, C), np.float32))
    filled = run_loss(users, cands, score, label, E, coef, pre)
    tag = "%s D%d x%g coef%g" % (name, D, scale, coef)
    on = E.astype(bool)
    _, mag = R.logits(users, np.nan_to_num(cands))
    check_sum("inbatch/z " + tag, got["z"][on], ref["z"][on], mag[on], D + 1)
    assert (got["z"][~on] == SENT).all(), "z written where E = 0"
    check("inbatch/per " + tag, got["per"], ref["per"], FWD)
    check("inbatch/target " + tag, got["losses"][1], ref["target"], FWD, 0.0)
    assert got["losses"][0] == SENT and (got["losses"][2:] == SENT).all()
    check("inbatch/dz " + tag, got["dz"], ref["dz"], DSCORE)
    assert (got["dz"][~on] == 0.0).all()
    check("inbatch/dscore " + tag, got["dscore"], ref["dscore_add"], DSCORE)
    assert (filled["dscore"].astype(np.float32) == pre + got["dscore"].astype(np.float32)).all(), "the distillation part did not survive"
    assert all((filled[k] == got[k]).all() for k in ("dz", "z", "per", "losses"))
    for k in got:
        assert np.isfinite(got[k]).all(), k


def test_loss_does_not_depend_on_the_position_in_the_batch():
    """The three impressions of fixture b3 alone, and as impressions 1, 3, 4 of a batch of five whose other impressions hold the
    padding news only: the same pairs give the same z bits, the same impressions the same loss."""
    D, C = 64, 2
    hist3, cand3 = R.fixture("b3")
    at = [1, 3, 4]
    hist5, cand5 = np.zeros((5, hist3.shape[1]), np.int32), np.zeros((5, C), np.int32)
    hist5[at], cand5[at] = hist3, cand3
    E3, E5 = R.eligibility(hist3, cand3), R.eligibility(hist5, cand5)
    slots = np.concatenate([np.arange(b * C, (b + 1) * C) for b in at])
    assert (E5[at][:, slots] == E3).all() and E5[at].sum() == E3.sum() and E3.sum() > 0
    users3, cands3, score3, label3 = rnd((3, D), 1), rnd((3 * C, D), 2), rnd((3, C), 3), np.array([1, 0, 1], np.int64)
    users5, cands5, score5, label5 = rnd((5, D), 4), rnd((5 * C, D), 5), rnd((5, C), 6), np.zeros(5, np.int64)
    users5[at], cands5[slots], score5[at], label5[at] = users3, cands3, score3, label3
    g3 = run_loss(users3, cands3, score3, label3, E3, 1.0, np.zeros((3, C), np.float32))
    g5 = run_loss(users5, cands5, score5, label5, E5, 1.0, np.zeros((5, C), np.float32))
    on = E3.astype(bool)
    assert (g5["z"][at][:, slots][on].astype(np.float32).view(np.int32) == g3["z"][on].astype(np.float32).view(np.int32)).all()
    assert (g5["per"][at].astype(np.float32).view(np.int32) == g3["per"].astype(np.float32).view(np.int32)).all()


@pytest.mark.parametrize("name,D", [("b5", 60), ("m65", 256), ("m600", 64)])
def test_logits_are_the_device_metrics_scores(name, D):
    """z[b, j] and the score tnr_rank_metrics writes for user row b and news row j: torch.equal."""
    users, cands, score, label, E = loss_inputs(name, D, 1.0, D, nan_rows=False)
    B, C = score.shape
    M = B * C
    z = torch.zeros((B, M), device=DEV)
    dscore, dz, per, losses = (torch.zeros(s, device=DEV) for s in ((B, C), (B, M), (B,), (4,)))
    T.call("tnr_inbatch_loss", dev(users), D, dev(cands), D, dev(score), dev(label), dev(R.words(E).view(np.int32)), 1.0, dscore, dz, z,
           per, losses, B, C, D)
    offs = dev((np.arange(B + 1) * M).astype(np.int32))
    cand = dev(np.tile(np.arange(M, dtype=np.int32), B))
    lab = torch.zeros(B * M, device=DEV, dtype=torch.int32)
    scores = torch.zeros(B * M, device=DEV)
    acc = torch.zeros(6, device=DEV, dtype=torch.float64)
    T.call("tnr_rank_metrics", dev(users), D, B, dev(cands), D, M, D, offs, cand, lab, scores, None, acc, 0)
    torch.cuda.synchronize()
    on = dev(E.astype(bool))
    assert int(on.sum()) > 0 and torch.equal(z[on], scores.view(B, M)[on])
    # rows one float apart from 16-byte alignment take the scalar loads: the same bits
    up, cp = torch.zeros((B, D + 1), device=DEV), torch.zeros((M, D + 1), device=DEV)
    up[:, :D], cp[:, :D] = dev(users), dev(cands)
    z2, per2 = torch.zeros((B, M), device=DEV), torch.zeros(B, device=DEV)
    T.call("tnr_inbatch_loss", up, D + 1, cp, D + 1, dev(score), dev(label), dev(R.words(E).view(np.int32)), 1.0, dscore, dz, z2,
           per2, losses, B, C, D)
    torch.cuda.synchronize()
    assert torch.equal(z2, z) and torch.equal(per2, per)


# ------------------------------------------------------------------------------------------------ tnr_inbatch_bwd
def run_bwd(dz, E, users, cands, pre_u, pre_c, C, pad=0):
    B, D = users.shape
    M = B * C
    z, words, u, v = dev(dz.astype(np.float32)), dev(R.words_v(E).view(np.int32)), strided(users, pad), strided(cands, pad)

    def fn():
        o = dict(duser=Buf(B, D, fill=pre_u), dcand=Buf(M, D, fill=pre_c))
        T.call("tnr_inbatch_bwd", z, words, u, D + pad, v, D + pad, o["duser"].t, o["dcand"].t, B, C, D)
        return o
    return twice(fn)


@pytest.mark.parametrize("name,D", [("s5", 4), ("b5", 60), ("b4", 260), ("m65", 256), ("m65", 68), ("m600", 64), ("m600", 516)])
def test_bwd(name, D):
    """D below, at and above the 256 threads of a workgroup; the outputs are added to; rows without a set bit keep their bits."""
    users, cands, score, label, E = loss_inputs(name, D, 1.0, D + 3)
    B, C = score.shape
    dz = R.loss(users, cands, score, label, E, 1.0)["dz"].astype(np.float32)
    want_u, want_c = R.bwd(dz, users, cands)
    pre_u, pre_c = rnd((B, D), 1, 1e-3), rnd((B * C, D), 2, 1e-3)
    inc = run_bwd(dz, E, users, cands, np.zeros_like(pre_u), np.zeros_like(pre_c), C)
    got = run_bwd(dz, E, users, cands, pre_u, pre_c, C)
    check("inbatch/duser %s D%d" % (name, D), inc["duser"], want_u, DVEC)
    check("inbatch/dcand %s D%d" % (name, D), inc["dcand"], want_c, DVEC)
    assert (got["duser"].astype(np.float32) == pre_u + inc["duser"].astype(np.float32)).all()
    assert (got["dcand"].astype(np.float32) == pre_c + inc["dcand"].astype(np.float32)).all()
    no_u, no_c = E.sum(1) == 0, E.sum(0) == 0
    assert no_u.any() and no_c.any()
    assert (got["duser"][no_u] == pre_u[no_u].astype(np.float64)).all() and (got["dcand"][no_c] == pre_c[no_c].astype(np.float64)).all()


def test_bwd_of_one_impression_writes_nothing():
    users, cands, score, label, E = loss_inputs("one", 64, 1.0, 5, nan_rows=False)
    pre_u, pre_c = rnd((1, 64), 1), rnd((5, 64), 2)
    got = run_bwd(np.zeros((1, 5)), E, users, cands, pre_u, pre_c, 5)
    assert (got["duser"] == pre_u.astype(np.float64)).all() and (got["dcand"] == pre_c.astype(np.float64)).all()


# ------------------------------------------------------------------------------------------------ at the kernels' limits
# inbatch_ref.LIMITS: 255 / 256 / 257 eligible slots per impression (the rank rounds of ib_loss_kernel's sum), 255 ... 513 slots
# (the slot rounds, ib_first_kernel's workgroups), 8192 slots (every LDS array of ib_loss_kernel full) and 8191.  The reference is
# the vectorised float64 one, which tests/test_inbatch_ref_cpu.py holds to the loops; the bounds are the ones above, unchanged.
_CASE = {}
PLAN_LIMITS = [(n, U) for n in R.LIMIT_FIXTURES for U in ((R.MAX_MIXED_U,) if n == "max_mixed" else (1, 3) if n == "w8191" else (1, 3, 50))]


@pytest.mark.parametrize("name,U", PLAN_LIMITS)
def test_plan_at_the_limits(name, U):
    hist, cand = R.limit_fixture(name, U)
    E = R.limit_eligibility(name, U)
    M = E.shape[1]
    got = run_plan(hist, cand)                                  # guards behind elig, count and first_ws; two runs, equal bits
    assert (got["elig"] == R.words_v(E)).all() and (got["count"].view(np.int32) == E.sum(1)).all()
    if M % 32:
        assert not (got["elig"][:, -1] >> np.uint32(M % 32)).any(), "bits past slot M - 1"


def limit_case(name, D, scale, coef):
    """Inputs of a limit fixture and their float64 loss, computed once: users scaled so that the logits have magnitude `scale`,
    NaN in every candidate row that is eligible for nobody."""
    key = (name, D, scale, coef)
    if key not in _CASE:
        hist, cand = R.limit_fixture(name)
        B, C = cand.shape
        E = R.limit_eligibility(name)
        seed = 11 * D + len(name) + B
        users, cands = rnd((B, D), seed, scale / np.sqrt(D)), rnd((B * C, D), seed + 1)
        cands[E.sum(0) == 0] = np.nan
        score = rnd((B, C), seed + 2, scale)
        label = np.random.RandomState(seed).randint(0, C, B).astype(np.int64)
        ref = R.loss_v(users, cands, score, label, E, coef)
        _CASE[key] = (users, cands, score, label, E, ref)
    return _CASE[key]


# (fixture, D, logit scale, coef, row padding in floats: 4 keeps the 16-byte loads, 1 takes the scalar ones)
LIMIT_LOSS = [("r255", 28, 1.0, 0.2, 4), ("r255", 1024, 30.0, 1.0, 0), ("r256", 32, 30.0, 1.0, 4), ("r256", 1020, 1.0, 0.2, 4),
              ("r257", 36, 1.0, 1.0, 1), ("r257", 64, 30.0, 0.2, 4), ("s256", 28, 30.0, 0.2, 4), ("s256", 1024, 1.0, 1.0, 4),
              ("s257", 32, 1.0, 0.2, 4), ("s257", 1020, 30.0, 1.0, 1), ("s513", 36, 30.0, 1.0, 4), ("s513", 256, 1.0, 0.2, 4),
              ("max", 1024, 30.0, 1.0, 4), ("max", 32, 1.0, 0.2, 4), ("max_mixed", 1024, 1.0, 0.2, 4), ("max_mixed", 36, 30.0, 1.0, 4)]


@pytest.mark.parametrize("name,D,scale,coef,pad", LIMIT_LOSS)
def test_loss_at_the_limits(name, D, scale, coef, pad):
    """test_loss's checks at the edges of the rounds and at 8192 slots, D at the edges of the 32-wide chunk and of the 1024-float
    user vector; NaN in the rows nobody is eligible for and behind every row; z requested and compared wherever E = 1."""
    users, cands, score, label, E, ref = limit_case(name, D, scale, coef)
    B, C = score.shape
    pre = rnd((B, C), D, 0.01)
    got = run_loss(users, cands, score, label, E, coef, np.zeros((B, C), np.float32), pad)
    filled = run_loss(users, cands, score, label, E, coef, pre, pad)
    tag = "%s D%d x%g coef%g" % (name, D, scale, coef)
    on = E.astype(bool)
    _, mag = R.logits(users, np.nan_to_num(cands))
    check_sum("inbatch/z " + tag, got["z"][on], ref["z"][on], mag[on], D + 1)
    assert (got["z"][~on] == SENT).all(), "z written where E = 0"
    check("inbatch/per " + tag, got["per"], ref["per"], FWD)
    check("inbatch/target " + tag, got["losses"][1], ref["target"], FWD, 0.0)
    assert got["losses"][0] == SENT and (got["losses"][2:] == SENT).all()
    check("inbatch/dz " + tag, got["dz"], ref["dz"], DSCORE)
    assert (got["dz"][~on] == 0.0).all()
    check("inbatch/dscore " + tag, got["dscore"], ref["dscore_add"], DSCORE)
    assert (filled["dscore"].astype(np.float32) == pre + got["dscore"].astype(np.float32)).all(), "the distillation part did not survive"
    assert all((filled[k] == got[k]).all() for k in ("dz", "z", "per", "losses"))
    for k in got:
        assert np.isfinite(got[k]).all(), k
    if name == "max_mixed":                                     # without the optional z: nothing else moves, z is not touched
        none = run_loss(users, cands, score, label, E, coef, np.zeros((B, C), np.float32), pad, want_z=False)
        assert (none["z"] == SENT).all() and all((none[k] == got[k]).all() for k in ("dz", "dscore", "per", "losses"))


# (fixture, D, coef of the loss whose dz is fed: the 1024-wide ones are test_loss_at_the_limits' cases, computed once)
LIMIT_BWD = [("r255", 4, 1.0), ("r256", 1028, 1.0), ("r257", 1020, 1.0), ("s256", 1024, 1.0), ("s257", 4, 1.0), ("s513", 1028, 1.0),
             ("max", 1024, 1.0), ("max", 4, 1.0), ("max_mixed", 1028, 0.2), ("max_mixed", 1024, 0.2), ("max_mixed", 4, 0.2)]


@pytest.mark.parametrize("name,D,coef", LIMIT_BWD)
def test_bwd_at_the_limits(name, D, coef):
    """D up to and over the 1024 the loss stops at (the backward takes any D); added to pre-filled buffers; rows without a set
    bit keep their bits (and the candidate rows among them hold NaN, which must not be read into anything)."""
    users, cands, score, label, E, ref = limit_case(name, min(D, 1024), 1.0, coef)
    if D > 1024:                                                # dz from the widest loss, rows widened for the backward alone
        users = np.concatenate([users, rnd((users.shape[0], D - 1024), D, 1.0 / 32)], 1)
        more = rnd((cands.shape[0], D - 1024), D + 1)
        more[E.sum(0) == 0] = np.nan
        cands = np.concatenate([cands, more], 1)
    B, C = score.shape
    dz = ref["dz"].astype(np.float32)
    want_u, want_c = R.bwd_v(dz, users, cands)
    pre_u, pre_c = rnd((B, D), 1, 1e-3), rnd((B * C, D), 2, 1e-3)
    inc = run_bwd(dz, E, users, cands, np.zeros_like(pre_u), np.zeros_like(pre_c), C, pad=4)
    got = run_bwd(dz, E, users, cands, pre_u, pre_c, C, pad=4)
    check("inbatch/duser %s D%d" % (name, D), inc["duser"], want_u, DVEC)
    check("inbatch/dcand %s D%d" % (name, D), inc["dcand"], want_c, DVEC)
    assert (got["duser"].astype(np.float32) == pre_u + inc["duser"].astype(np.float32)).all()
    assert (got["dcand"].astype(np.float32) == pre_c + inc["dcand"].astype(np.float32)).all()
    no_u, no_c = E.sum(1) == 0, E.sum(0) == 0
    assert name not in ("max_mixed", "s256", "s257", "s513") or no_c.any()
    assert name != "max_mixed" or no_u.any()
    assert (got["duser"][no_u] == pre_u[no_u].astype(np.float64)).all() and (got["dcand"][no_c] == pre_c[no_c].astype(np.float64)).all()


def test_loss_does_not_depend_on_the_position_in_a_large_batch():
    """The first three impressions of r257 (C = 1) alone, and as impressions 1, 300 and 511 of a batch of 512 whose other
    impressions hold the padding news only: their slots sit in the first and the second round of 256, the same pairs give the
    same z bits and the same impressions the same loss bits."""
    D, C = 64, 1
    hist, cand = R.limit_fixture("r257")
    hist3, cand3 = hist[:3], cand[:3]
    at = [1, 300, 511]
    histN, candN = np.zeros((512, hist3.shape[1]), np.int32), np.zeros((512, C), np.int32)
    histN[at], candN[at] = hist3, cand3
    E3, EN = R.eligibility_v(hist3, cand3), R.eligibility_v(histN, candN)
    assert (EN[at][:, at] == E3).all() and EN[at].sum() == E3.sum() == 6      # (the padding impressions rank against the three too)
    users3, cands3, score3, label3 = rnd((3, D), 1), rnd((3, D), 2), rnd((3, C), 3), np.zeros(3, np.int64)
    usersN, candsN, scoreN, labelN = rnd((512, D), 4), rnd((512, D), 5), rnd((512, C), 6), np.zeros(512, np.int64)
    usersN[at], candsN[at], scoreN[at] = users3, cands3, score3
    g3 = run_loss(users3, cands3, score3, label3, E3, 1.0, np.zeros((3, C), np.float32))
    gN = run_loss(usersN, candsN, scoreN, labelN, EN, 1.0, np.zeros((512, C), np.float32))
    on = E3.astype(bool)
    f32 = lambda x: torch.from_numpy(np.ascontiguousarray(x).astype(np.float32))
    assert torch.equal(f32(gN["z"][at][:, at][on]), f32(g3["z"][on]))
    assert torch.equal(f32(gN["per"][at]), f32(g3["per"]))
    check("inbatch/per of three", g3["per"], R.loss_v(users3, cands3, score3, label3, E3, 1.0)["per"], FWD)


@pytest.mark.parametrize("bad", [-1, 16, 200])
def test_loss_with_a_label_out_of_range(bad):
    """Fixture r256 (B 17, C 16), impression 5's label outside [0, C): its loss and losses[1] are NaN; every other impression's
    per, dz and dscore row has the bits of the run with a valid label; nothing is written behind any buffer (run_loss's guards).
    200 is a label that has a thread of its own in the workgroup, in another wave than thread 0."""
    users, cands, score, label, E, ref = limit_case("r256", 32, 30.0, 1.0)
    B, C = score.shape
    zeros = np.zeros((B, C), np.float32)
    good = run_loss(users, cands, score, label, E, 1.0, zeros)
    lab = label.copy()
    lab[5] = bad
    got = run_loss(users, cands, score, lab, E, 1.0, zeros)
    others = np.arange(B) != 5
    assert np.isnan(got["per"][5]) and np.isnan(got["losses"][1]) and not np.isnan(good["losses"][1])
    for k in ("per", "dz", "dscore", "z"):
        assert (got[k][others] == good[k][others]).all(), k
    assert (got["dz"][5] == good["dz"][5]).all() and np.isfinite(got["dscore"][5]).all()
    check("inbatch/dscore of the bad row", got["dscore"][5], R.loss_v(users, cands, score, lab, E, 1.0)["dscore_add"][5], DSCORE)


# ------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize("B,C,D,word", [(8193, 1, 64, "8192"), (4, 5, 1028, "1024"), (4, 5, 6, "multiple of 4"), (4, 17, 64, "16"),
                                        (512, 16, 1028, "1024"), (481, 17, 1024, "16"), (2731, 3, 1024, "8192")])
def test_loss_refuses_and_writes_nothing(B, C, D, word):
    """Refused on the host before anything is launched: the buffers are never dereferenced, so small ones do."""
    o = [Buf(64) for _ in range(5)]
    src = torch.zeros(64, device=DEV)
    with pytest.raises(T.TnrError, match=word):
        T.call("tnr_inbatch_loss", src, D, src, D, src, torch.zeros(8, device=DEV, dtype=torch.int64), src.view(torch.int32), 1.0,
               o[0].t, o[1].t, o[2].t, o[3].t, o[4].t, B, C, D)
    torch.cuda.synchronize()
    assert all(bool((x.raw == SENT).all()) for x in o)
