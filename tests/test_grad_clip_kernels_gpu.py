"""The kernels of global-norm gradient clipping (csrc/optim.hip: tnr_grad_sumsq_scan, tnr_grad_clip_commit,
tnr_amsgrad_step_clipped), one by one, against the float64 references of tests/clip_ref.py and tests/heads_ref.py, with the Buf /
twice idiom of tests/test_heads_kernels_gpu.py: a sentinel region behind every output must come back untouched and two runs must
give the same bits (include/tnr_hip.h promises a fixed order).

Bounds.
  * Sum of squares: relative (c + 1) * 2^-23, c = clip_ref.sumsq_depth(n), the longest chain of fp32 additions a term passes
    through in grad_sumsq_kernel as written: 4 per trip of the grid-stride loop in the lane's running sum of its component (one
    trip up to n = 2048 * 4096, two behind it), + 2 for (s0 + s1) + (s2 + s3), + 6 for the wave butterfly, + 3 for the four waves
    in wave order: c = 15 for one trip, 19 for two.  The sum over the partials is in double and adds nothing.  It is a ceiling on
    the error, not a description of it: every comparison prints its error as a fraction of the bound.
  * Coefficient and norm: relative 1e-6 (behind the double sum there are the conversions to fp32 and one divide).
  * tnr_amsgrad_step_clipped: p rtol 1e-5, atol 1e-6 (the optimiser tests' bound); m, v, vmax rtol 1e-5 with a floor of 1e-5 of
    the buffer's largest magnitude - the first Adam step is scale-free in p, so the state is where clipping shows."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import clip_ref as C                                    # noqa: E402
import heads_ref as R                                   # noqa: E402
import tnr_hip as T                                     # noqa: E402
from test_heads_kernels_gpu import Buf, twice, rnd, dev, host, check, check_abs, HYPER     # noqa: E402

DEV = "cuda:0"
N_TWO_TRIPS = C.GRID_CAP * C.BLOCK + 4096 + 1027        # second trip of the grid-stride loop: one full block + a ragged tail
SIZES = [1, 3, 4, 1023, 4095, 4096, 4097, 3 * 4096 + 5, N_TWO_TRIPS]
_CACHE = {}


def grad(n, seed=11):
    """N(0, 1e-3^2) values (shared, never modified) -> (fp32 numpy, device tensor with 16-byte-aligned storage)."""
    if (n, seed) not in _CACHE:
        x = rnd((n,), seed, 1e-3)
        _CACHE[(n, seed)] = (x, dev(x))
    return _CACHE[(n, seed)]


def report(what, got, want, rtol):
    err = abs(got - want)
    print("[grad-clip] %s: got %.9g, float64 %.9g, rel err %.3e, err / bound %.4f" % (what, got, want, err / abs(want), err / (rtol * abs(want))))
    assert np.isfinite(got) and err <= rtol * abs(want), what


def scan_commit(slices, max_norm, gs=1.0, guard=None, stamp=0):
    """tnr_grad_sumsq_scan over every device slice, the partials one behind the other, then one tnr_grad_clip_commit."""
    parts = [T.query("tnr_grad_sumsq_parts", t.numel()) for t in slices]
    part, clip = Buf(sum(parts)), Buf(2)
    off = 0
    for t, k in zip(slices, parts):
        T.call("tnr_grad_sumsq_scan", t, t.numel(), part.t[off:], guard, stamp)
        off += k
    T.call("tnr_grad_clip_commit", part.t, off, max_norm, gs, clip.t)
    return {"part": part, "clip": clip}


@pytest.mark.parametrize("n", SIZES)
def test_sum_of_squares_against_float64(n):
    x, t = grad(n)
    out = twice(lambda: scan_commit([t], 1.0))
    want = float((x.astype(np.float64) ** 2).sum())
    assert out["part"].shape == (C.sumsq_parts(n),)
    rtol = C.sumsq_rtol([n])
    report("sum of the partials n%d (c = %d)" % (n, C.sumsq_depth(n)), float(out["part"].sum()), want, rtol)
    report("norm^2 n%d" % n, float(out["clip"][1]) ** 2, want, rtol + 2.0 ** -23)      # + the norm's own rounding to fp32 (2^-24), squared


def test_sum_of_squares_in_pieces():
    """Disjoint 16-byte-aligned slices whose boundaries are no multiples of 4096, one commit over the concatenated partials."""
    n = 3 * 4096 + 5
    x, t = grad(n)
    cuts = [0, 4, 1000, 4100, 8196 + 8, n]
    slices = [t[a:b] for a, b in zip(cuts, cuts[1:])]
    assert all(s.data_ptr() % 16 == 0 for s in slices)
    out = twice(lambda: scan_commit(slices, 1.0))
    want = float((x.astype(np.float64) ** 2).sum())
    rtol = C.sumsq_rtol([b - a for a, b in zip(cuts, cuts[1:])])
    report("sum of the partials of %d pieces" % len(slices), float(out["part"].sum()), want, rtol)
    report("norm^2 over %d pieces" % len(slices), float(out["clip"][1]) ** 2, want, rtol + 2.0 ** -23)


@pytest.mark.parametrize("gs", [1.0, 0.5])
def test_coefficient_and_norm(gs):
    n = 4097
    x, t = grad(n)
    true = gs * float(np.sqrt((x.astype(np.float64) ** 2).sum()))
    for f in (0.5, 1.0 - 1e-3, 1.0 + 1e-3, 2.0):
        max_norm = float(np.float32(f * true))
        out = twice(lambda: scan_commit([t], max_norm, gs))["clip"]
        total, coef = C.clip([x], max_norm, gs)
        report("norm gs%g thr %gx" % (gs, f), float(out[1]), total, 1e-6)
        report("coef gs%g thr %gx" % (gs, f), float(out[0]), coef, 1e-6)
        assert (coef == 1.0) == (f > 1.0)
        if f == 2.0:
            assert out[0] == 1.0                              # exactly 1.0f: the clipped update is then the unclipped one, bit for bit


def test_overflowing_sum_gives_inf_and_zero():
    """One FINITE element of 3e19: its square overflows fp32 -> norm = inf, coefficient = 0, as torch's fp32 computation."""
    x = grad(4097)[0].copy()
    x[2050] = 3e19
    t = dev(x)
    out = twice(lambda: scan_commit([t], 1.0))["clip"]
    assert np.isposinf(out[1]) and out[0] == 0.0
    g32 = torch.from_numpy(x)
    assert torch.isinf((g32 * g32).sum().sqrt())


@pytest.mark.parametrize("n", [4096 + 1027, N_TWO_TRIPS])
def test_fused_scan_raises_the_guard_as_the_plain_scan_does(n):
    x, _ = grad(n)
    tail = n - 3                                              # inside the ragged tail (n is no multiple of 4096)
    for where, val in ((None, 0.0), (0, np.inf), (n - 1, np.nan), (tail, -np.inf)):
        y = x
        if where is not None:
            y = x.copy()
            y[where] = val
        t = dev(y) if where is not None else grad(n)[1]
        ga = torch.tensor([3, 1, 0, 0], dtype=torch.int32, device=DEV)
        gb = ga.clone()
        T.call("tnr_grad_nonfinite_scan", t, n, ga, 7)
        out = scan_commit([t], 1.0, guard=gb, stamp=7)
        torch.cuda.synchronize()
        assert out["part"].guard_ok() and out["clip"].guard_ok()
        assert torch.equal(ga, gb), (where, ga.tolist(), gb.tolist())
        assert ga.tolist() == ([3, 1, 0, 0] if where is None else [7, 1, 0, 0])       # a clean slice never touches it


def _state(n, ams):
    return [Buf(n, fill=rnd((n,), 5)), Buf(n, fill=0.0), Buf(n, fill=0.0), Buf(n, fill=0.0) if ams else None]


@pytest.mark.parametrize("ams", [1, 0])
@pytest.mark.parametrize("n", [5, 4099])
def test_amsgrad_step_clipped_three_steps(n, ams):
    gs = 0.5
    grads = [rnd((n,), 900 + s, sc) for s, sc in enumerate((1e-3, 1e-1, 1e-4))]
    max_norm = float(np.float32(0.85 * gs * np.sqrt((grads[0].astype(np.float64) ** 2).sum())))    # 0.85 of step 1's norm: clips steps 1 and 2 only
    coefs = [C.clip([g], max_norm, gs)[1] for g in grads]
    assert coefs[0] < 1.0 and coefs[1] < 1.0 and coefs[2] == 1.0

    def fn():
        st = _state(n, ams)
        trace = []
        for s in range(3):
            g = dev(grads[s])
            c = scan_commit([g], max_norm, gs)["clip"]
            T.call("tnr_amsgrad_step_clipped", st[0].t, g, st[1].t, st[2].t, st[3].t if ams else None, n, s + 1, *HYPER, gs,
                   None, 0, 0, c.t)
            trace.append([host(b.t) for b in st if b is not None])
        return {k: b for k, b in zip("pmvx", [b for b in st if b is not None])}, trace
    (a, ta), (b, tb) = fn(), fn()
    torch.cuda.synchronize()
    for k in a:
        assert a[k].guard_ok() and b[k].guard_ok() and torch.equal(a[k].t, b[k].t)
    ref = [R.f64(rnd((n,), 5)), np.zeros(n), np.zeros(n), np.zeros(n) if ams else None]
    for s in range(3):
        ref = list(R.adam_step(ref[0], grads[s], ref[1], ref[2], ref[3], s + 1, *HYPER, grad_scale=gs * coefs[s]))
        for name, got, want in zip("pmvx", ta[s], [r for r in ref if r is not None]):
            what = "clipped/%s n%d ams%d step%d" % (name, n, ams, s + 1)
            if name == "p":
                check_abs(what, got, want, 1e-5, 1e-6)
            else:
                check(what, got, want, 1e-5, 1e-5)


@pytest.mark.parametrize("ams", [1, 0])
@pytest.mark.parametrize("n", [5, 4099])
def test_amsgrad_step_clipped_with_coefficient_one_is_the_guarded_step(n, ams):
    g = dev(rnd((n,), 9))
    one = torch.tensor([1.0, 123.0], dtype=torch.float32, device=DEV)
    outs = []
    for clipped in (False, True):
        st = _state(n, ams)
        for b, sd in zip(st[1:], (6, 7, 8)):
            if b is not None:
                b.t.copy_(dev(np.abs(rnd((n,), sd, 0.1)) + (0.05 if sd == 8 else 0.0)))
        guard = torch.tensor([3, 4, 0, 0], dtype=torch.int32, device=DEV)
        args = (st[0].t, g, st[1].t, st[2].t, st[3].t if ams else None, n, 5, *HYPER, 0.125, guard, 7, 3)
        if clipped:
            T.call("tnr_amsgrad_step_clipped", *args, one)
        else:
            T.call("tnr_amsgrad_step_guarded", *args)
        torch.cuda.synchronize()
        assert all(b.guard_ok() for b in st if b is not None)
        outs.append([b.t.clone() for b in st if b is not None])
    assert all(torch.equal(x, y) for x, y in zip(*outs))
    # stamp == guard[0]: the skipped step touches nothing, whatever the coefficient
    st = _state(n, ams)
    before = [b.t.clone() for b in st if b is not None]
    guard = torch.tensor([9, 1, 0, 0], dtype=torch.int32, device=DEV)
    half = torch.tensor([0.5, 1.0], dtype=torch.float32, device=DEV)
    T.call("tnr_amsgrad_step_clipped", st[0].t, g, st[1].t, st[2].t, st[3].t if ams else None, n, 5, *HYPER, 1.0, guard, 9, 0, half)
    torch.cuda.synchronize()
    assert all(torch.equal(x, b.t) and b.guard_ok() for x, b in zip(before, [b for b in st if b is not None]))
    assert not torch.equal(outs[0][0], before[0])
