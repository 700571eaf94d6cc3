"""tnr_grad_accum (csrc/optim.hip: grad_accum_kernel<OVERWRITE>), the streaming pass of gradient accumulation, with the Buf sentinel
and run-twice idiom of tests/test_heads_kernels_gpu.py.

No tolerance anywhere: overwrite != 0 copies, overwrite == 0 makes ONE correctly rounded IEEE fp32 add per element, so the result
has numpy's float32 bits (`a + b`, respectively `b`).  Non-finite results are compared by class (inf with its sign, or NaN: payloads
are not part of the promise), every finite position bit for bit.

Sizes: the optimiser kernels' (scalar tail, one 16-byte access, the 1024-element sub-blocks, one element past a full 4096 block)
plus both sides of one and two full blocks, and CAP * 4096 + 4097 = one full trip of the capped grid, one more full block and one
element: the grid-stride loop's second, partial trip."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import tnr_hip as T                                     # noqa: E402
from test_heads_kernels_gpu import Buf, dev             # noqa: E402
from test_adamw_kernels_gpu import SIZES as OPT_SIZES   # noqa: E402

CAP = 2048                                              # ACCUM_GRID_CAP of csrc/optim.hip
BIG = CAP * 4096 + 4097
SIZES = OPT_SIZES + [4095, 4096, 8191, 8193, BIG]
_CACHE = {}


def inputs(n):
    """(a, b): N(0, 1) draws with exact zeros of both signs mixed in (about one element in 8 each); shared, never modified."""
    if n not in _CACHE:
        out = []
        for seed in (11, 12):
            r = np.random.RandomState(seed)
            x = r.standard_normal(n).astype(np.float32)
            k = r.randint(0, 8, n)
            x[k == 0] = 0.0
            x[k == 1] = -0.0
            out.append(x)
        _CACHE[n] = tuple(out)
    return _CACHE[n]


def bits(x):
    if isinstance(x, torch.Tensor):
        x = x.cpu().numpy()
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def run(a, b, overwrite):
    """dst (a Buf filled with a) <- accum(dst, src = b): -> (dst Buf, src Buf)."""
    n = a.size
    dst, src = Buf(n, fill=a), Buf(n, fill=b)
    T.call("tnr_grad_accum", dst.t, src.t, n, overwrite)
    return dst, src


def run_twice(a, b, overwrite):
    (d0, s0), (d1, s1) = run(a, b, overwrite), run(a, b, overwrite)
    torch.cuda.synchronize()
    for x in (d0, s0, d1, s1):
        assert x.guard_ok(), "wrote behind a buffer"
    assert np.array_equal(bits(d0.t), bits(d1.t)), "two runs differ"
    assert np.array_equal(bits(s0.t), bits(b)) and np.array_equal(bits(s1.t), bits(b)), "src was modified"
    return d0.t.cpu().numpy()


def same(what, got, want):
    """finite positions bit for bit, non-finite ones by class"""
    fin = np.isfinite(want)
    assert np.array_equal(np.isfinite(got), fin), "%s: finite / non-finite positions differ" % what
    bad = np.flatnonzero(bits(got)[fin] != bits(want)[fin])
    assert bad.size == 0, "%s: %d finite elements differ, first at %d" % (what, bad.size, np.flatnonzero(fin)[bad[0]])
    assert np.array_equal(np.isnan(got), np.isnan(want)), "%s: NaN positions differ" % what
    inf = np.isinf(want)
    assert np.array_equal(np.sign(got[inf]), np.sign(want[inf])), "%s: an infinity changed its sign" % what


@pytest.mark.parametrize("n", SIZES)
def test_add_and_overwrite_have_numpy_float32_bits(n):
    a, b = inputs(n)
    got = run_twice(a, b, 0)
    assert np.array_equal(bits(got), bits(a + b)), "dst + src"
    got = run_twice(a, b, 1)
    assert np.array_equal(bits(got), bits(b)), "overwrite"


@pytest.mark.parametrize("n", [5, 4097, 8193])
def test_overwrite_does_not_read_a_nan_filled_destination(n):
    _, b = inputs(n)
    got = run_twice(np.full(n, np.nan, np.float32), b, 1)
    assert np.array_equal(bits(got), bits(b))


def _positions(n):
    """first, last, a tail element (behind the last full 4096 block; the vector body's last one when there is no tail) and the
    elements on both sides of every 4096 boundary"""
    pos = {0, n - 1, max(n - 2, 0), (n // 4096) * 4096 - 1 if n >= 4096 else n // 2}
    for k in range(4096, n, 4096):
        pos |= {k - 1, k}
    return sorted(p for p in pos if 0 <= p < n)


@pytest.mark.parametrize("where", ["src", "dst", "both"])
@pytest.mark.parametrize("n", [5, 4097, 8193 + 4096])
def test_non_finite_values_propagate_as_ieee_addition_does(n, where):
    a, b = (x.copy() for x in inputs(n))
    vals = [np.inf, -np.inf, np.nan]
    for i, p in enumerate(_positions(n)):
        if where in ("src", "both"):
            b[p] = vals[i % 3]
        if where in ("dst", "both"):
            a[p] = vals[(i + (1 if i % 2 else 0)) % 3]          # even i: the same value, odd i: inf + -inf and inf + nan pairs
    if where == "both":                                          # inf + -inf -> NaN, whatever the positions above paired
        a[n // 2], b[n // 2] = np.inf, -np.inf
    with np.errstate(invalid="ignore"):
        want = a + b
    if where == "both":
        assert np.isnan(want[n // 2])
    assert (~np.isfinite(want)).sum() >= min(3, n - 1)
    same("add/%s" % where, run_twice(a, b, 0), want)
    same("overwrite/%s" % where, run_twice(a, b, 1), b)


def test_a_slice_36_elements_into_a_larger_buffer():
    n, off = 4097 + 33, 36
    a, b = inputs(n + off + 20)
    dst, src = Buf(a.size, fill=a), Buf(b.size, fill=b)
    for ow in (0, 1):
        T.call("tnr_grad_accum", dst.t[off:off + n], src.t[off:off + n], n, ow)
        torch.cuda.synchronize()
        want = a.copy()
        want[off:off + n] = b[off:off + n] if ow else a[off:off + n] + b[off:off + n]
        assert np.array_equal(bits(dst.t), bits(want)), "overwrite=%d: the slice or its surroundings" % ow
        assert np.array_equal(bits(src.t), bits(b)) and dst.guard_ok() and src.guard_ok()
        dst.t.copy_(dev(a))


def test_bad_arguments_are_errors_not_launches():
    n = 4097
    a, b = inputs(n)
    dst, src = Buf(n, fill=a), Buf(n, fill=b)
    for what, args in (("NULL dst", (None, src.t, n, 0)), ("NULL src", (dst.t, None, n, 0)), ("n = 0", (dst.t, src.t, 0, 0)),
                       ("n < 0", (dst.t, src.t, -4, 1)), ("dst off by 4 bytes", (dst.t[1:], src.t, n - 1, 0)),
                       ("src off by 4 bytes", (dst.t, src.t[1:], n - 1, 1)), ("dst == src", (dst.t, dst.t, n, 0)),
                       ("dst == src, overwrite", (src.t, src.t, n, 1))):
        with pytest.raises(T.TnrError) as err:
            T.call("tnr_grad_accum", *args)
        assert "(-1)" in str(err.value) and "tnr_grad_accum" in str(err.value).split("): ", 1)[1], what     # TNR_EINVAL + message
        torch.cuda.synchronize()
        assert np.array_equal(bits(dst.t), bits(a)) and np.array_equal(bits(src.t), bits(b)), what
        assert dst.guard_ok() and src.guard_ok(), what
