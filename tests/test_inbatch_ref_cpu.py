"""CPU: tests/inbatch_ref.py, the float64 reference the in-batch-negatives GPU tests compare against, is tied down here - its
gradients to torch autograd on the same extended cross-entropy, its E = 0 case to heads_ref.kd_score_loss, its mask to a
hand-worked example - and every id fixture of the GPU tests is held to the fixture condition (conditions on the inputs: a fixture
that does not meet them would let a kernel that skips a rule pass)."""
import numpy as np
import pytest
import torch

import heads_ref as HR
import inbatch_ref as R


def _inputs(name, D, seed, scale=1.0):
    hist, cand = R.fixture(name)
    B, C = cand.shape
    rs = np.random.RandomState(seed)
    users = rs.standard_normal((B, D)) * scale
    cands = rs.standard_normal((B * C, D))
    score = rs.standard_normal((B, C)) * scale
    label = rs.randint(0, C, B)
    return users, cands, score, label, R.eligibility(hist, cand)


@pytest.mark.parametrize("name", ["b3", "b4", "b5", "m65"])
@pytest.mark.parametrize("coef", [0.2, 1.0])
def test_gradients_against_autograd(name, coef):
    users, cands, score, label, E = _inputs(name, 8, 3)
    B, C = score.shape
    ref = R.loss(users, cands, score, label, E, coef)
    du, dc = R.bwd(ref["dz"], users, cands)
    u, v, s = (torch.tensor(x, dtype=torch.float64, requires_grad=True) for x in (users, cands, score))
    z = u @ v.T
    z.retain_grad()
    per = []
    for b in range(B):
        lg = torch.cat([s[b], z[b][torch.from_numpy(E[b].astype(bool))]])
        per.append(-torch.log_softmax(lg, 0)[int(label[b])])
    per = torch.stack(per)
    (coef * per.mean()).backward()
    np.testing.assert_allclose(ref["per"], per.detach().numpy(), rtol=1e-12, atol=1e-12)
    assert abs(ref["target"] - float(per.detach().mean())) < 1e-12
    np.testing.assert_allclose(ref["dscore_add"], s.grad.numpy(), rtol=1e-10, atol=1e-14)
    np.testing.assert_allclose(ref["dz"], z.grad.numpy(), rtol=1e-10, atol=1e-14)
    assert (ref["dz"][E == 0] == 0).all() and (ref["dz"][E == 1] > 0).all()
    np.testing.assert_allclose(du, u.grad.numpy(), rtol=1e-10, atol=1e-14)
    np.testing.assert_allclose(dc, v.grad.numpy(), rtol=1e-10, atol=1e-14)
    np.testing.assert_allclose(ref["z"][E == 1], z.detach().numpy()[E == 1], rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("coef", [0.2, 1.0])
def test_no_negatives_is_the_plain_target_loss(coef):
    users, cands, score, label, E = _inputs("b5", 8, 4, scale=3.0)
    ref = R.loss(users, cands, score, label, np.zeros_like(E), coef)
    plain = HR.kd_score_loss(score, None, label, 1.0, coef)
    assert abs(ref["target"] - plain["target"]) < 1e-12
    np.testing.assert_allclose(ref["dscore_add"], plain["dscore"], rtol=1e-12, atol=1e-15)
    assert not ref["dz"].any()
    one = R.loss(users[:1], cands[:2], score[:1], label[:1], R.eligibility(np.zeros((1, 3)), np.array([[4, 5]])), coef)     # B = 1
    assert abs(one["target"] - HR.kd_score_loss(score[:1], None, label[:1], 1.0, coef)["target"]) < 1e-12


def test_hand_worked_example():
    """Three impressions, C = 2, U = 2.  Slots 0..5 hold 5 7 | 7 0 | 9 5.
      rule 2: slot 3 (id 0) is nobody's.  rule 3: slot 2 (7 again) and slot 5 (5 again) are nobody's.
      impression 0 (own 5 7, clicked 9 0): slots 2..5 are foreign; 2, 3, 5 are out; slot 4 (9) is clicked: rule 5 -> none.
      impression 1 (own 7 0, clicked 1 2): slots 0, 1, 4, 5 are foreign; slot 1 (7) is its own news too: rule 4; 5 out -> 0, 4.
      impression 2 (own 9 5, clicked 0 0): slots 0..3 are foreign; slot 0 (5) is its own news too: rule 4; 2, 3 out -> 1."""
    hist = np.array([[9, 0], [1, 2], [0, 0]], np.int32)
    cand = np.array([[5, 7], [7, 0], [9, 5]], np.int32)
    want = np.array([[0, 0, 0, 0, 0, 0], [1, 0, 0, 0, 1, 0], [0, 1, 0, 0, 0, 0]], np.uint8)
    E = R.eligibility(hist, cand)
    assert (E == want).all(), E
    assert (R.words(E) == np.array([[0], [0b10001], [0b10]], np.uint32)).all()
    st = R.eligibility(hist, cand, stages=True)
    assert [int(s.sum()) for s in st] == [12, 10, 6, 4, 3]
    # bit 31 / 32 of the words: slot 32 is the first bit of the second word
    E2 = np.zeros((1, 33), np.uint8)
    E2[0, 31] = E2[0, 32] = 1
    assert (R.words(E2) == np.array([[0x80000000, 1]], np.uint32)).all()


# ------------------------------------------------------------------------------------- the vectorised forms and the limit fixtures
@pytest.mark.parametrize("name", R.FIXTURES)
def test_vectorised_forms_equal_the_loops(name):
    """eligibility_v / words_v exactly (every stage), loss_v / bwd_v to 1e-12 of the loops, on every fixture the loops can do;
    NaN in the rows nobody is eligible for must not reach the vectorised results (the loops never read those rows)."""
    hist, cand = R.fixture(name)
    st, sv = R.eligibility(hist, cand, stages=True), R.eligibility_v(hist, cand, stages=True)
    assert all(a.dtype == b.dtype and (a == b).all() for a, b in zip(st, sv))
    E = st[4]
    assert (R.eligibility_v(hist, cand) == E).all()
    wl, wv = R.words(E), R.words_v(E)
    assert wl.dtype == wv.dtype == np.uint32 and wl.shape == wv.shape and (wl == wv).all()
    for coef, scale in ((0.2, 1.0), (1.0, 30.0)):
        users, cands, score, label, _ = _inputs(name, 12, 5, scale)
        dead = cands.copy()
        dead[E.sum(0) == 0] = np.nan
        a, b = R.loss(users, cands, score, label, E, coef), R.loss_v(users, dead, score, label, E, coef)
        assert abs(a["target"] - b["target"]) <= 1e-12 * abs(a["target"])
        for k in ("per", "dscore_add", "dz"):
            np.testing.assert_allclose(b[k], a[k], rtol=1e-12, atol=1e-300, err_msg=k)
        _, mag = R.logits(users, cands)
        assert (np.abs(a["z"] - b["z"]) <= 1e-12 * mag).all() and (b["z"][E == 0] == 0).all()
        du, dc = R.bwd(a["dz"], users, cands)
        dv, dcv = R.bwd_v(a["dz"], users, dead)
        mu, mc = np.abs(a["dz"]) @ np.abs(cands), np.abs(a["dz"]).T @ np.abs(users)
        assert (np.abs(du - dv) <= 1e-12 * mu).all() and (np.abs(dc - dcv) <= 1e-12 * mc).all()
        assert np.isfinite(dv).all() and np.isfinite(dcv).all()


def test_vectorised_loss_with_a_label_out_of_range():
    """The kernel's convention: that impression's loss and the mean are NaN, everything else is as with a valid label."""
    users, cands, score, label, E = _inputs("b5", 8, 4)
    good = R.loss_v(users, cands, score, label, E, 1.0)
    for y in (-1, 2, 200):
        lab = label.copy()
        lab[2] = y
        bad = R.loss_v(users, cands, score, lab, E, 1.0)
        others = np.arange(5) != 2
        assert np.isnan(bad["per"][2]) and np.isnan(bad["target"]) and (bad["per"][others] == good["per"][others]).all()
        assert (bad["dz"] == good["dz"]).all() and (bad["dscore_add"][others] == good["dscore_add"][others]).all()
        assert np.isfinite(bad["dscore_add"]).all() and (bad["dscore_add"][2] > 0).all()


@pytest.mark.parametrize("name", R.LIMIT_FIXTURES)
def test_limit_fixtures_are_what_the_table_says(name):
    """Slots, eligible slots per impression, and what each fixture exists for - asserted on the inputs, so that a fixture that
    slid off its edge fails here and not silently."""
    B, C, _, _, per = R.LIMITS[name]
    for U in ((R.MAX_MIXED_U,) if name == "max_mixed" else (1, 3) if name == "w8191" else (1, 3, 50)):
        hist, cand = R.limit_fixture(name, U)
        assert hist.shape == (B, U) and cand.shape == (B, C) and hist.dtype == cand.dtype == np.int32
        assert hist.min() >= 0 and cand.min() >= 0 and B * C == R.LIMIT_SLOTS[name] <= 8192 and C <= 16
        assert R.limit_fixture(name, U)[1] is cand                                       # built once
        st = R.eligibility_v(hist, cand, stages=True)
        E = st[4]
        if per is not None:
            assert (E.sum(1) == per).all() and per == (B - 1) * C
        elif name != "max_mixed":
            removed = [bool((st[r - 1] > st[r]).any()) for r in range(1, 5)]
            assert all(removed[1:]), (name, U, removed)                                  # rules 3 - 5 all fire
            assert E.sum(1).max() > 0 and np.unique(E.sum(1)).size > 1
    if name == "max":
        assert ((R.words_v(E) == 0xFFFFFFFF).sum(1) == 255).all()                       # all 256 words in use: one's own is half set
    if name == "max_mixed":
        cond = R.max_mixed_conditions(E)
        assert all(cond.values()), cond
        removed = [bool((st[r - 1] > st[r]).any()) for r in range(1, 5)]
        assert all(removed), removed
        assert (st[2][:, 32:64].sum(0) == 511).all() and not st[1][:, 64:96].any()
    if name == "w8191":
        assert R.words_v(E).shape == (8191, 256) and not (R.words_v(E)[:, 255] >> np.uint32(31)).any()


def test_the_rank_rounds_of_the_limit_fixtures():
    """ib_loss_kernel's `for (r = tid; r < n_elig; r += 256)`: 255, 256, 257 ranks; 8176 = 31 full rounds and one of 240."""
    got = {n: int(R.limit_eligibility(n).sum(1).max()) for n in ("r255", "r256", "r257", "max")}
    assert got == {"r255": 255, "r256": 256, "r257": 257, "max": 8176}
    assert R.limit_eligibility("r255") is R.limit_eligibility("r255")


@pytest.mark.parametrize("name", R.FIXTURES)
def test_fixture_condition(name):
    """Every id fixture of tests/test_inbatch_kernels_gpu.py and tests/test_inbatch_gpu.py (the shapes that are degenerate by
    design - B = 1, all-distinct ids, the plan's word-edge sweep - are checked there against eligibility() itself)."""
    hist, cand = R.fixture(name)
    cond = R.condition(hist, cand)
    assert all(cond.values()), (name, cond)
    assert hist.dtype == np.int32 and cand.dtype == np.int32 and hist.min() >= 0 and cand.min() >= 0
