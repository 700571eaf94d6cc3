"""tnr_adamw_step_ema (csrc/optim.hip: amsgrad_kernel<AMS, CLIP, WD, EMA = true>) against the float64 reference of tests/ema_ref.py,
with the Buf / run_twice idiom and the inputs of tests/test_adamw_kernels_gpu.py: a sentinel region behind every buffer, the average
included, must come back untouched and two runs must give the same bits.

Bounds: that file's for p, m, v, vmax (p rtol 1e-5, atol 1e-6; m, v, vmax rtol 1e-5 with a floor of 1e-5 of the buffer's largest
magnitude) and the p bound for the average: the new average is a convex combination of the old one (exact) and p_new, so its error
is at most p_new's, plus the three fp32 roundings of e + w (p_new - e): the difference and w itself (2^-24 of w |p_new - e| each)
and the fma's result (2^-24 of |e_new|).  With both inputs N(0, 1), |p_new - e| stays below ~6 over 4097 elements, so the three
together stay below ~1e-6 where the bound 1e-6 + 1e-5 |e_new| is at its smallest, and an order below it at typical magnitudes.
Beside the bound, p, m, v, vmax must be BIT-equal to tnr_adamw_step's on the same inputs: the average changes nothing else."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import ema_ref as M                                     # noqa: E402
import tnr_hip as T                                     # noqa: E402
from test_heads_kernels_gpu import Buf, rnd, dev, host, check_abs     # noqa: E402
from test_adamw_kernels_gpu import (DEV, SIZES, LR, B1, B2, EPS, WD, masks, bits, inputs, fresh, run, reference,     # noqa: E402
                                    compare)

WS = (1.0, 0.5, 0.1, 0.0)
_E = {}


def ema0(n):
    """The average before the step: N(0, 1), another draw than p's; shared and never modified."""
    if n not in _E:
        _E[n] = rnd((n,), 11)
    return _E[n]


def run_ema(n, ams, lrs, wd, wbits, first, ws, step=3, gs=0.5, guard=None, stamp=0, known=0, clip=None):
    st = fresh(n, ams)
    e = Buf(n, fill=ema0(n))
    g = dev(inputs(n)[1])
    T.call("tnr_adamw_step_ema", st[0].t, g, st[1].t, st[2].t, st[3].t if ams else None, n, step, lrs[0], lrs[1], lrs[2], B1, B2, EPS,
           gs, wd, wbits, first, guard, stamp, known, clip, e.t, ws[0], ws[1], ws[2])
    out = dict(zip("pmvx", [b for b in st if b is not None]))
    out["e"] = e
    return out


def run_ema_twice(*a, **kw):
    x, y = run_ema(*a, **kw), run_ema(*a, **kw)
    torch.cuda.synchronize()
    for k in x:
        assert x[k].guard_ok() and y[k].guard_ok(), "%s: wrote behind its buffer" % k
        assert torch.equal(x[k].t.view(torch.int32), y[k].t.view(torch.int32)), "%s: two runs differ" % k
    return {k: x[k].t.clone() for k in x}


def compare_all(what, got, want_pmvx, w):
    compare(what, {k: v for k, v in got.items() if k != "e"}, want_pmvx)
    check_abs("%s/ema" % what, host(got["e"]), M.ema_step(ema0(got["e"].numel()), want_pmvx["p"], w), 1e-5, 1e-6)


def same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("ams", [1, 0])
@pytest.mark.parametrize("n", SIZES)
def test_sizes_against_float64_and_the_update_keeps_its_bits(n, ams):
    """Every size x (decay through the `runs` mask at first = 0 and 36, no decay) x (clip given, NULL) x w in {1, 0.5, 0.1, 0}: all
    five buffers against float64, and p, m, v, vmax bit-equal to tnr_adamw_step on the same inputs."""
    half = torch.tensor([0.5, 123.0], dtype=torch.float32, device=DEV)
    mask = masks()["runs"]
    wb = bits(mask)
    lrs = (LR, LR, LR)
    for wd, wbits, first in ((WD, wb, 0), (WD, wb, 36), (0.0, None, 0)):
        for clip in (None, half):
            want = reference(n, ams, LR, wd, mask[first:first + n], 3, 0.5 * (0.5 if clip is not None else 1.0))
            base = run(n, ams, lrs, wd, wbits, first, clip=clip)
            for w in WS:
                got = run_ema_twice(n, ams, lrs, wd, wbits, first, (w, w, w), clip=clip)
                compare_all("ema n%d ams%d wd%g first%d clip%d w%g" % (n, ams, wd, first, clip is not None, w), got, want, w)
                for k in base:
                    assert same_bits(got[k], base[k].t), (k, wd, first, w)
                if w == 0.0:
                    assert same_bits(got["e"], dev(ema0(n)))                 # e + 0 (p - e): the average's own bits
    # the average shows: w = 0.5 lands far from both the old average and the new parameters
    got = run_ema(n, ams, lrs, 0.0, None, 0, (0.5, 0.5, 0.5))
    assert not same_bits(got["e"].t, dev(ema0(n))) and not same_bits(got["e"].t, got["p"].t)


@pytest.mark.parametrize("ams", [1, 0])
@pytest.mark.parametrize("n", [5, 1025])
def test_guard_picks_the_weight_with_the_rate_and_skips_the_average(n, ams):
    """A crafted guard word: guard[1] - known_skips = 0, 1, 2, 3 picks w0, w1, w2, w2 together with lr0, lr1, lr2, lr2 and the bias
    corrections of step, step - 1, step - 2, step - 2; guard[0] == stamp leaves all five buffers bit-unchanged."""
    lrs, ws = (1e-2, 7e-3, 4e-3), (0.9, 0.5, 0.1)
    mask = masks()["runs"]
    wb = bits(mask)
    seen = []
    for k in (0, 1, 2, 3):
        guard = torch.tensor([3, 4 + k, 0, 0], dtype=torch.int32, device=DEV)
        got = run_ema_twice(n, ams, lrs, WD, wb, 36, ws, step=5, guard=guard, stamp=7, known=4)
        want = reference(n, ams, lrs[min(k, 2)], WD, mask[36:36 + n], 5 - min(k, 2), 0.5)
        compare_all("ema guard k%d n%d ams%d" % (k, n, ams), got, want, ws[min(k, 2)])
        seen.append(got["e"])
        assert guard.tolist() == [3, 4 + k, 0, 0]
    assert not same_bits(seen[0], seen[1]) and not same_bits(seen[1], seen[2]) and same_bits(seen[2], seen[3])
    # the weight alone (one rate): the pick still follows the guard
    for k in (0, 1, 2, 3):
        guard = torch.tensor([3, 4 + k, 0, 0], dtype=torch.int32, device=DEV)
        got = run_ema_twice(n, ams, (LR, LR, LR), 0.0, None, 0, ws, step=5, guard=guard, stamp=7, known=4)
        want = reference(n, ams, LR, 0.0, False, 5 - min(k, 2), 0.5)
        compare_all("ema guard (weight only) k%d n%d ams%d" % (k, n, ams), got, want, ws[min(k, 2)])
    # the skipped step: nothing moves, nothing decays, the average keeps its bits
    guard = torch.tensor([9, 1, 0, 0], dtype=torch.int32, device=DEV)
    half = torch.tensor([0.5, 1.0], dtype=torch.float32, device=DEV)
    for clip in (None, half):
        got = run_ema_twice(n, ams, lrs, WD, bits(masks()["all"]), 0, ws, step=5, guard=guard, stamp=9, known=0, clip=clip)
        p, g, m, v, x = inputs(n)
        for k, want in zip("pmvxe", (p, m, v, x, ema0(n))):
            if k in got:
                assert same_bits(got[k], dev(want)), k


def test_bad_arguments_are_errors_not_launches():
    n = 33
    st = fresh(n, 1)
    e = Buf(n + 4, fill=ema0(n + 4))
    g = dev(inputs(n)[1])
    wb = bits(masks()["all"])
    bufs = st + [e]
    before = [b.t.clone() for b in bufs]
    head = (st[0].t, g, st[1].t, st[2].t, st[3].t, n, 1)
    mid = (LR, LR, LR, B1, B2, EPS, 1.0)
    ok = (0.0, None, 0, None, 0, 0, None)                    # weight_decay .. clip of a legal call without decay
    nan = float("nan")
    cases = [("ema == NULL", ok + (None, 0.1, 0.1, 0.1)),
             ("ema not 16-byte aligned", ok + (e.t[1:], 0.1, 0.1, 0.1)),
             ("w0 < 0", ok + (e.t, -0.1, 0.1, 0.1)), ("w1 < 0", ok + (e.t, 0.1, -1e-6, 0.1)), ("w2 < 0", ok + (e.t, 0.1, 0.1, -2.0)),
             ("w0 > 1", ok + (e.t, 1.5, 0.1, 0.1)), ("w1 > 1", ok + (e.t, 0.1, 1.0001, 0.1)), ("w2 > 1", ok + (e.t, 0.1, 0.1, 1e9)),
             ("w0 NaN", ok + (e.t, nan, 0.1, 0.1)), ("w1 NaN", ok + (e.t, 0.1, nan, 0.1)), ("w2 NaN", ok + (e.t, 0.1, 0.1, nan)),
             # ... and everything tnr_adamw_step refuses
             ("first % 4 != 0", (WD, wb, 2, None, 0, 0, None, e.t, 0.1, 0.1, 0.1)),
             ("first % 4 != 0 without decay", (0.0, None, 6, None, 0, 0, None, e.t, 0.1, 0.1, 0.1)),
             ("first < 0", (WD, wb, -4, None, 0, 0, None, e.t, 0.1, 0.1, 0.1)),
             ("NULL map with weight_decay > 0", (WD, None, 0, None, 0, 0, None, e.t, 0.1, 0.1, 0.1)),
             ("weight_decay < 0", (-0.1, wb, 0, None, 0, 0, None, e.t, 0.1, 0.1, 0.1))]
    for what, tail in cases:
        with pytest.raises(T.TnrError):
            T.call("tnr_adamw_step_ema", *head, *mid, *tail)
        torch.cuda.synchronize()
        assert all(torch.equal(a, b.t) and b.guard_ok() for a, b in zip(before, bufs)), what
    for what, bad in (("n < 1", (st[0].t, g, st[1].t, st[2].t, st[3].t, 0, 1)), ("step < 1", (st[0].t, g, st[1].t, st[2].t, st[3].t, n, 0)),
                      ("p == NULL", (None, g, st[1].t, st[2].t, st[3].t, n, 1))):
        with pytest.raises(T.TnrError):
            T.call("tnr_adamw_step_ema", *bad, *mid, *ok, e.t, 0.1, 0.1, 0.1)
        torch.cuda.synchronize()
        assert all(torch.equal(a, b.t) and b.guard_ok() for a, b in zip(before, bufs)), what
    # the bounds themselves are legal: w = 0 and w = 1
    T.call("tnr_adamw_step_ema", *head, *mid, *ok, e.t, 0.0, 1.0, 1.0)
    torch.cuda.synchronize()
    assert not torch.equal(before[0], st[0].t) and torch.equal(before[4], e.t) and e.guard_ok()
