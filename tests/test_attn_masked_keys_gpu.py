"""The short-title attention kernels (csrc/attn.hip: tnr_attn_l32_fwd / _bwd and their _do forms) do not load the K and V rows of
keys the mask zeroes.  A key j of sequence n is dead iff mask_add[n][j] - max_k mask_add[n][k] <= -9000 (live_keys in attn.hip;
the precondition stands beside tnr_attn_l32_fwd in include/tnr_hip.h): relative to the row's own maximum, so an all-padding
sequence has no dead key.

N = 6 sequences, A = 3 heads, L in {1, 30, 32}, both 16-bit builds.  Sequence by sequence the live keys are: none (every key
-10000: all of them count), the first 1, 2, L - 1 and L keys, and a mask with holes (keys 0, 3 and L - 1 live), all cut to L.
  1. ctx, dq, dk, dv and the bias partials against the float64 reference of tests/attn_ref.py under the bounds and the Frobenius check
     of tests/test_attn_kernels_gpu.py (attn_ref.failures, unchanged), and with dropout p = 0.1 through the _do entry points against
     dropout_ref under the tolerances of tests/test_dropout_kernels_gpu.py.
  2. NaN in the K and V rows of the dead keys changes no output (np.array_equal, everything finite), while in the same launch NaN in
     one V row of the all-padding sequence - a live row - comes out as NaN.
  3. Finite values of magnitude 100 in the dead rows against zeros there: equal outputs."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import attn_ref as AR                          # noqa: E402
import dropout_ref as DR                       # noqa: E402
import rows_ref as RR                          # noqa: E402
import test_attn_kernels_gpu as TA             # noqa: E402
import test_dropout_kernels_gpu as TD          # noqa: E402
import tnr_hip as T                            # noqa: E402

DEV = "cuda:0"
N, A, D = 6, 3, AR.D
HD = A * D
LS = (1, 30, 32)
DEAD_BELOW = -9000.0
P_DROP = 0.1
TD_DTYPE = {"bf16": "bf16", "f16": "fp16"}     # rows_ref's kinds -> test_dropout_kernels_gpu's build names


def live_sets(L):
    """The live keys of the six sequences (an empty set = every key padded)."""
    cut = lambda ks: sorted({k for k in ks if 0 <= k < L})
    return [[], cut(range(1)), cut(range(2)), cut(range(L - 1)), cut(range(L)), cut((0, 3, L - 1))]


@functools.lru_cache(maxsize=None)
def case(L, kind):
    """attn_ref's plain inputs at (N, L, A) under this file's masks, the float64 reference, its bounds and the rounding model:
    computed once, shared, never modified.  dead (N, L) bool follows the rule above."""
    c = AR.Case("l32", N, L, A, "plain")
    inp = AR.inputs(c, kind)
    madd = np.full((N, 32), AR.NEG_INF, AR.F32)
    madd[:, :L] = AR.PAD
    for n, ks in enumerate(live_sets(L)):
        madd[n, ks] = 0.0
    inp = dict(inp, mask_add=madd)
    dead = (madd.astype(np.float64) - madd.max(1, keepdims=True).astype(np.float64) <= DEAD_BELOW)[:, :L]
    assert not dead[0].any() and (L == 1 or dead[1:4].any(1).all()), "the all-padding sequence has no dead key, the short ones do"
    r = AR.reference(inp)
    return c, inp, dead, r, AR.bounds(r, kind, "l32"), AR.emulate(kind, "l32", inp)


def run(kind, qkv, dctx, inp, L, p=0.0):
    """Forward + backward through the C ABI (p > 0: the _do entry points) on device tensors qkv / dctx -> {name: float64 numpy}."""
    td, sfx = RR.tdtype(kind), RR.SFX[kind]
    madd, rel = TA.dev32(inp["mask_add"]), TA.dev32(inp["rel"])
    o = dict(ctx=TA.Buf(N * L, HD, dtype=td), dqkv=TA.Buf(N * L, 3 * HD, dtype=td), bias_part=TA.Buf(N, 3 * HD))
    if p:
        st = TD.site(p, T.DROP_PROB)
        T.call("tnr_attn_l32_fwd_do" + sfx, qkv, madd, rel, o["ctx"].t, N, L, A, st)
        T.call("tnr_attn_l32_bwd_do" + sfx, qkv, madd, rel, dctx, o["dqkv"].t, o["bias_part"].t, N, L, A, st)
    else:
        T.call("tnr_attn_l32_fwd" + sfx, qkv, madd, rel, o["ctx"].t, N, L, A)
        T.call("tnr_attn_l32_bwd" + sfx, qkv, madd, rel, dctx, o["dqkv"].t, o["bias_part"].t, N, L, A)
    torch.cuda.synchronize()
    assert all(b.guard_ok() for b in o.values()), "wrote behind an output"
    return {n: TA.host(b.t) for n, b in o.items()}


def with_dead_rows(inp, dead, kind, fill):
    """qkv on the device with fill(shape) in the K and V columns (every head) of the dead keys' rows."""
    qkv = TA.dev_rows(inp["qkv"], RR.tdtype(kind))
    rows = torch.from_numpy(np.flatnonzero(dead.reshape(-1))).to(DEV)
    if len(rows):
        qkv[rows, HD:] = fill((len(rows), 2 * HD)).to(qkv.dtype)
    return qkv


@pytest.mark.parametrize("kind", RR.KINDS)
@pytest.mark.parametrize("L", LS)
def test_masked_keys_against_float64(L, kind):
    c, inp, dead, r, b, emu = case(L, kind)
    d = TA.device_inputs(inp, kind)
    got, _ = TA.twice(lambda: TA.launch("l32", kind, d, N, L, A))
    bad, _ = AR.failures(kind, inp, r, b, got, emu, tag="masked-keys " + AR.case_id(c))
    assert not bad, (AR.case_id(c), kind, bad)


@pytest.mark.parametrize("kind", RR.KINDS)
@pytest.mark.parametrize("L", LS)
def test_masked_keys_with_dropout_against_float64(L, kind):
    """p = 0.1 through the _do entry points: ctx, all of dqkv and the bias partials under test_dropout_kernels_gpu's tolerances."""
    c, inp, dead, _, _, _ = case(L, kind)
    tol_f, tol_b = [t / (1.0 - P_DROP) for t in TD.ATTN_TOL["l32"][TD_DTYPE[kind]]]
    td = RR.tdtype(kind)
    got = run(kind, TA.dev_rows(inp["qkv"], td), TA.dev_rows(inp["dctx"], td), inp, L, p=P_DROP)
    ref = DR.attn_fwd(inp["qkv"], inp["mask_add"][:, :L], inp["rel"][:, :L, :L], N, L, A, m=TD.probs_mask(P_DROP, N, A, L))
    want_d, _ = DR.attn_bwd(ref, inp["dctx"])
    tag = "masked-keys %s %s p=%.1f" % (AR.case_id(c), kind, P_DROP)
    TD.check(tag + " ctx", got["ctx"], ref["ctx"], tol_f, tol_f)
    scale = np.abs(want_d).max()
    TD.check(tag + " dqkv", got["dqkv"], want_d, tol_b, tol_b * scale)
    TD.check(tag + " bias partials", got["bias_part"].sum(0), got["dqkv"].sum(0), 1e-3, 1e-3 * scale * N * L)


@pytest.mark.parametrize("p", [0.0, P_DROP])
@pytest.mark.parametrize("kind", RR.KINDS)
@pytest.mark.parametrize("L", LS)
def test_dead_rows_are_not_read(L, kind, p):
    c, inp, dead, _, _, _ = case(L, kind)
    td = RR.tdtype(kind)
    dctx = TA.dev_rows(inp["dctx"], td)
    first = run(kind, TA.dev_rows(inp["qkv"], td), dctx, inp, L, p)
    qkv = with_dead_rows(inp, dead, kind, lambda s: torch.full(s, float("nan"), device=DEV))
    qkv[0, 2 * HD:] = float("nan")                  # V row of key 0 of the all-padding sequence, every head: a live row
    second = run(kind, qkv, dctx, inp, L, p)
    for n in first:
        per_seq = lambda x: x.reshape(N, -1)
        a, s = per_seq(first[n]), per_seq(second[n])
        assert np.isfinite(a).all() and np.isfinite(s[1:]).all(), (n, "not finite")
        assert np.array_equal(a[1:], s[1:]), (n, "NaN in a dead K / V row changed an output")
    # every query of the all-padding sequence spreads its probability over every key; under dropout a query keeps key 0 with
    # probability 0.9 per head, so some element is NaN in any case
    ctx0 = second["ctx"].reshape(N, -1)[0]
    assert np.isnan(ctx0).all() if p == 0.0 else np.isnan(ctx0).any(), "a live V row of the all-padding sequence was not read"


@pytest.mark.parametrize("kind", RR.KINDS)
@pytest.mark.parametrize("L", LS)
def test_dead_rows_do_not_matter(L, kind):
    c, inp, dead, _, _, _ = case(L, kind)
    td = RR.tdtype(kind)
    dctx = TA.dev_rows(inp["dctx"], td)
    sign = lambda s: torch.where(torch.rand(s, device=DEV, generator=torch.Generator(DEV).manual_seed(L)) < 0.5, -100.0, 100.0)
    big = run(kind, with_dead_rows(inp, dead, kind, sign), dctx, inp, L)
    zero = run(kind, with_dead_rows(inp, dead, kind, lambda s: torch.zeros(s, device=DEV)), dctx, inp, L)
    for n in big:
        assert np.isfinite(big[n]).all(), n
        assert np.array_equal(big[n], zero[n]), (n, "the values in dead K / V rows reached an output")
