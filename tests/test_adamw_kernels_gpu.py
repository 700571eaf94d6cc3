"""tnr_adamw_step (csrc/optim.hip: amsgrad_kernel<AMS, CLIP, WD>) against the float64 reference of tests/adamw_ref.py, with the Buf /
twice idiom of tests/test_heads_kernels_gpu.py: a sentinel region behind every output must come back untouched and two runs must
give the same bits.

Bounds: the optimiser tests' own - p rtol 1e-5, atol 1e-6; m, v, vmax rtol 1e-5 with a floor of 1e-5 of the buffer's largest
magnitude.  The decay adds one fp32 multiply by 1 - lr wd (2^-24 relative, the factor itself formed from a double product rounded
once), which is inside the p bound.  Every comparison prints its error as a fraction of the bound."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import adamw_ref as A                                   # noqa: E402
import tnr_hip as T                                     # noqa: E402
from test_heads_kernels_gpu import Buf, rnd, dev, host, check, check_abs, HYPER     # noqa: E402

DEV = "cuda:0"
SIZES = [1, 3, 4, 5, 31, 32, 33, 1023, 1024, 1025, 4097]
FIRSTS = [0, 4, 36, 1028]
MAP_N = 1028 + 4097 + 75                                # the map is longer than every slice: elements behind first + n exist
LR, B1, B2, EPS = HYPER
WD = 0.1
_CACHE = {}


def masks():
    """name -> bool[MAP_N]: all, none, and runs whose boundaries fall at non-multiples of 4 and of 32 (and a single element)."""
    if "m" not in _CACHE:
        runs = np.zeros(MAP_N, bool)
        for a, b in ((1, 3), (6, 7), (13, 37), (62, 67), (95, 97), (129, 1027), (1029, 1030), (1061, 2050), (2051, 4099), (5101, 5127)):
            runs[a:b] = True
        _CACHE["m"] = {"all": np.ones(MAP_N, bool), "none": np.zeros(MAP_N, bool), "runs": runs}
    return _CACHE["m"]


def bits(mask):
    return torch.from_numpy(A.pack(mask).view(np.int32)).to(DEV)


def inputs(n):
    """p, g (N(0, 1) and N(0, 1e-1^2)) and a state in mid-training: m, v > 0, vmax >= v; shared and never modified."""
    if n not in _CACHE:
        _CACHE[n] = (rnd((n,), 5), rnd((n,), 9, 0.1), rnd((n,), 6, 0.1), np.abs(rnd((n,), 7, 0.1)),
                     np.abs(rnd((n,), 8, 0.1)) + 0.05)
    return _CACHE[n]


def fresh(n, ams):
    p, g, m, v, x = inputs(n)
    return [Buf(n, fill=p), Buf(n, fill=m), Buf(n, fill=v), Buf(n, fill=x) if ams else None]


def run(n, ams, lrs, wd, wbits, first, step=3, gs=0.5, guard=None, stamp=0, known=0, clip=None, entry="tnr_adamw_step"):
    st = fresh(n, ams)
    g = dev(inputs(n)[1])
    head = (st[0].t, g, st[1].t, st[2].t, st[3].t if ams else None, n, step)
    if entry == "tnr_adamw_step":
        T.call(entry, *head, lrs[0], lrs[1], lrs[2], B1, B2, EPS, gs, wd, wbits, first, guard, stamp, known, clip)
    elif entry == "tnr_amsgrad_step":
        T.call(entry, *head, lrs[0], B1, B2, EPS, gs)
    elif entry == "tnr_amsgrad_step_guarded":
        T.call(entry, *head, lrs[0], B1, B2, EPS, gs, guard, stamp, known)
    else:
        T.call(entry, *head, lrs[0], B1, B2, EPS, gs, guard, stamp, known, clip)
    return dict(zip("pmvx", [b for b in st if b is not None]))


def run_twice(*a, **kw):
    x, y = run(*a, **kw), run(*a, **kw)
    torch.cuda.synchronize()
    for k in x:
        assert x[k].guard_ok() and y[k].guard_ok(), "%s: wrote behind its buffer" % k
        assert torch.equal(x[k].t.view(torch.int32), y[k].t.view(torch.int32)), "%s: two runs differ" % k
    return {k: x[k].t.clone() for k in x}


def reference(n, ams, lr, wd, mask, step, gs):
    p, g, m, v, x = inputs(n)
    out = A.adamw_step(p, g, m, v, x if ams else None, step, lr, mask, wd, B1, B2, EPS, grad_scale=gs)
    return dict(zip("pmvx", [r for r in out if r is not None]))


def compare(what, got, want):
    for k in got:
        if k == "p":
            check_abs("%s/p" % what, host(got[k]), want[k], 1e-5, 1e-6)
        else:
            check("%s/%s" % (what, k), host(got[k]), want[k], 1e-5, 1e-5)


@pytest.mark.parametrize("ams", [1, 0])
@pytest.mark.parametrize("n", SIZES)
def test_sizes_masks_and_offsets_against_float64(n, ams):
    """Every size x every mask x every `first`, with and without a clip coefficient, against float64 AdamW on the slice's bits
    mask[first : first + n]."""
    half = torch.tensor([0.5, 123.0], dtype=torch.float32, device=DEV)
    for mname, mask in masks().items():
        wb = bits(mask)
        for first in FIRSTS:
            for clip in (None, half):
                gs = 0.5
                got = run_twice(n, ams, (LR, LR, LR), WD, wb, first, gs=gs, clip=clip)
                want = reference(n, ams, LR, WD, mask[first:first + n], 3, gs * (0.5 if clip is not None else 1.0))
                compare("adamw n%d ams%d mask-%s first%d clip%d" % (n, ams, mname, first, clip is not None), got, want)
    # the decay is visible at this size of lr * wd (1e-3 relative, 100x the bound), in the decayed elements only
    a = run(n, ams, (LR, LR, LR), WD, bits(masks()["all"]), 0)["p"].t
    b = run(n, ams, (LR, LR, LR), WD, bits(masks()["none"]), 0)["p"].t
    assert not torch.equal(a, b)


@pytest.mark.parametrize("ams", [1, 0])
@pytest.mark.parametrize("n", [5, 1025])
def test_zero_rate_moves_the_state_only(n, ams):
    """lr0 = 0 (the first update of a warmup): the decay factor is 1 - 0 x wd = 1 and the update 0, so p keeps its bits, whatever
    the mask; m and v (and vmax) still move, as torch's do."""
    got = run_twice(n, ams, (0.0, LR, LR), WD, bits(masks()["all"]), 4)
    assert torch.equal(got["p"], dev(inputs(n)[0]))
    want = reference(n, ams, 0.0, WD, True, 3, 0.5)
    compare("adamw lr0=0 n%d ams%d" % (n, ams), got, want)
    assert not torch.equal(got["m"], dev(inputs(n)[2])) and not torch.equal(got["v"], dev(inputs(n)[3]))


@pytest.mark.parametrize("ams", [1, 0])
@pytest.mark.parametrize("n", [5, 1025])
def test_guard_picks_rate_decay_and_bias_correction_together(n, ams):
    """A crafted guard word: guard[1] - known_skips = 0, 1, 2, 3 picks lr0, lr1, lr2, lr2 (with the bias corrections of step,
    step - 1, step - 2, step - 2 and the decay factor of the same rate); guard[0] == stamp leaves p, m, v, vmax bit-identical."""
    lrs = (1e-2, 7e-3, 4e-3)
    mask = masks()["runs"]
    wb = bits(mask)
    seen = []
    for k in (0, 1, 2, 3):
        guard = torch.tensor([3, 4 + k, 0, 0], dtype=torch.int32, device=DEV)
        got = run_twice(n, ams, lrs, WD, wb, 36, step=5, guard=guard, stamp=7, known=4)
        want = reference(n, ams, lrs[min(k, 2)], WD, mask[36:36 + n], 5 - min(k, 2), 0.5)
        compare("adamw guard k%d n%d ams%d" % (k, n, ams), got, want)
        seen.append(got["p"])
        assert guard.tolist() == [3, 4 + k, 0, 0]
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2]) and torch.equal(seen[2], seen[3])
    # never below step 1
    guard = torch.tensor([3, 2, 0, 0], dtype=torch.int32, device=DEV)
    got = run_twice(n, ams, lrs, WD, wb, 36, step=2, guard=guard, stamp=7, known=0)
    compare("adamw guard step2 k2 n%d ams%d" % (n, ams), got, reference(n, ams, lrs[2], WD, mask[36:36 + n], 1, 0.5))
    # the skipped step: nothing moves, nothing decays
    guard = torch.tensor([9, 1, 0, 0], dtype=torch.int32, device=DEV)
    half = torch.tensor([0.5, 1.0], dtype=torch.float32, device=DEV)
    got = run_twice(n, ams, lrs, WD, bits(masks()["all"]), 0, step=5, guard=guard, stamp=9, known=0, clip=half)
    p, g, m, v, x = inputs(n)
    for k, want in zip("pmvx", (p, m, v, x)):
        if k in got:
            assert torch.equal(got[k], dev(want)), k


@pytest.mark.parametrize("ams", [1, 0])
@pytest.mark.parametrize("n", [5, 1025, 4097])
def test_bit_identities_with_the_existing_entry_points(n, ams):
    """weight_decay = 0 with a NULL map and lr0 = lr1 = lr2 is tnr_amsgrad_step / _guarded / _clipped on the same inputs, bit for
    bit; so is weight_decay > 0 with an all-clear map (the WD instantiation, no element selected)."""
    guard = torch.tensor([3, 5, 0, 0], dtype=torch.int32, device=DEV)
    clip = torch.tensor([0.625, 9.0], dtype=torch.float32, device=DEV)
    none = bits(masks()["none"])
    cases = (("tnr_amsgrad_step", dict()),
             ("tnr_amsgrad_step_guarded", dict(guard=guard, stamp=7, known=4)),
             ("tnr_amsgrad_step_clipped", dict(guard=guard, stamp=7, known=4, clip=clip)),
             ("tnr_amsgrad_step_clipped", dict(clip=clip)))
    for entry, kw in cases:
        old = run_twice(n, ams, (LR, LR, LR), 0.0, None, 0, step=5, entry=entry, **kw)
        for wd, wb, first in ((0.0, None, 0), (0.0, None, 36), (WD, none, 0), (WD, none, 1028)):
            new = run_twice(n, ams, (LR, LR, LR), wd, wb, first, step=5, **kw)
            for k in old:
                assert torch.equal(old[k].view(torch.int32), new[k].view(torch.int32)), (entry, wd, first, k)
        assert not torch.equal(old["p"], dev(inputs(n)[0]))


def test_bad_arguments_are_errors_not_launches():
    n = 33
    st = fresh(n, 1)
    g = dev(inputs(n)[1])
    wb = bits(masks()["all"])
    before = [b.t.clone() for b in st]
    head = (st[0].t, g, st[1].t, st[2].t, st[3].t, n, 1)
    for what, tail in (("first % 4 != 0", (LR, LR, LR, B1, B2, EPS, 1.0, WD, wb, 2, None, 0, 0, None)),
                       ("first % 4 != 0 without decay", (LR, LR, LR, B1, B2, EPS, 1.0, 0.0, None, 6, None, 0, 0, None)),
                       ("first < 0", (LR, LR, LR, B1, B2, EPS, 1.0, WD, wb, -4, None, 0, 0, None)),
                       ("NULL map with weight_decay > 0", (LR, LR, LR, B1, B2, EPS, 1.0, WD, None, 0, None, 0, 0, None)),
                       ("weight_decay < 0", (LR, LR, LR, B1, B2, EPS, 1.0, -0.1, wb, 0, None, 0, 0, None))):
        with pytest.raises(T.TnrError):
            T.call("tnr_adamw_step", *head, *tail)
        torch.cuda.synchronize()
        assert all(torch.equal(a, b.t) and b.guard_ok() for a, b in zip(before, st)), what
    T.call("tnr_adamw_step", *head, LR, LR, LR, B1, B2, EPS, 1.0, 0.0, wb, 0, None, 0, 0, None)      # a map with weight_decay == 0: legal, unread
    torch.cuda.synchronize()
    assert not torch.equal(before[0], st[0].t)
