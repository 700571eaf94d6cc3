"""tnr_sgemm and tnr_sgemm_group (csrc/heads.hip: sgemm_tile, sgemm_kernel, sgemm_group_kernel and the two split-K reduce
kernels) against the float64 reference of tests/sgemm_ref.py, at tile and k-step edges, in every stride form and caller layout,
split and unsplit, alone and grouped.

Every case: the destination is a flat buffer (sentinel, or C0 where beta != 0, or NaN) with sentinel guards in front and behind;
a split case gets a partial buffer of exactly sgemm_ref.part_elems floats with a guard behind it; the case runs twice and the two
results have equal bits; every element outside the contract's written set (guards, ldc and sC gaps) comes back with the bits it
had; every written element is finite and within the DERIVED bound of the float64 value (gamma_n of an fp32 fma chain,
n = K + slices + 3, sgemm_ref.apply; tests/test_sgemm_ref_cpu.py shows that bound is neither too tight for an fp32 chain nor too
wide to see a dropped k, a shifted bias or a wrong leading dimension).  Every comparison prints its largest error and the worst
error / bound (EXPERIMENTS.md item 79 records them).  No case has a time assertion."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import sgemm_ref as R                          # noqa: E402
import tnr_hip as T                            # noqa: E402

DEV = "cuda:0"
SENT, GUARD = R.SENT, R.GUARD


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def bits(t):
    return t.detach().cpu().numpy().view(np.int32)


class Loaded:
    """A problem's operands on the device (one upload per distinct buffer: views of one buffer stay views of one buffer)."""

    def __init__(self, p):
        self.p = p
        self.A = dev(p["A"])
        self.B = self.A if p["B"] is p["A"] else dev(p["B"])
        self.bias = None if p["bias"] is None else dev(p["bias"])
        self.pe = R.part_elems(p)

    def fresh(self, c0):
        """-> (destination, partial buffer or None), new for every run."""
        part = torch.full((self.pe + GUARD,), SENT, device=DEV) if self.p["ksplit"] > 1 else None
        return dev(c0), part

    def fields(self, c, part):
        """The problem with device addresses: what tnr_sgemm_problem_t holds."""
        p = self.p
        q = {k: p[k] for k in R.FIELDS if k not in ("A", "B", "C", "bias", "part")}
        q.update(A=self.A.data_ptr() + 4 * p["a_off"], B=self.B.data_ptr() + 4 * p["b_off"], C=c.data_ptr() + 4 * p["c_off"],
                 bias=None if self.bias is None else self.bias.data_ptr() + 4 * p["bias_off"], part=part)
        return q

    def check_part(self, what, part):
        if part is None:
            return
        raw = part.cpu().numpy()
        assert (raw[self.pe:] == SENT).all(), "%s: wrote behind the %d floats of its partial buffer" % (what, self.pe)
        assert (raw[:self.pe] != SENT).all(), "%s: the slices do not fill the partial buffer (sgemm_ref.effective_split)" % what


def sgemm(q):
    T.call("tnr_sgemm", q["A"], q["a_rs"], q["a_cs"], q["sA"], None, q["B"], q["b_rs"], q["b_cs"], q["sB"], q["C"], q["ldc"], q["sC"],
           q["bias"], q["sBias"], q["M"], q["N"], q["K"], q["batch"], q["alpha"], q["beta"], q["ksplit"], q["part"])


def judge(what, got_bits, c0, ref):
    """got_bits: the destination's int32 image after the call; ref = sgemm_ref.apply(c0, p)."""
    want, bound, written = ref
    same = got_bits[~written] == c0.view(np.int32)[~written]
    assert same.all(), "%s: %d elements outside the written set changed (first at flat index %d)" % (
        what, int((~same).sum()), int(np.nonzero(~written)[0][np.argmin(same)]))
    got = got_bits.view(np.float32).astype(np.float64)[written]
    err = np.abs(got - want[written])
    with np.errstate(invalid="ignore"):
        ratio = np.where(err == 0.0, 0.0, err / bound[written])
    worst = float(np.nanmax(ratio, initial=0.0)) if np.isfinite(got).all() else float("nan")
    print("[sgemm-kernels] %s: max|err| %.3e, worst err / bound %.4f" % (what, float(np.nanmax(err, initial=0.0)), worst))
    assert np.isfinite(got).all(), "%s: %d written elements are not finite" % (what, int((~np.isfinite(got)).sum()))
    assert (err <= bound[written]).all(), "%s: %d of %d elements over the bound, worst err / bound %.3f" % (
        what, int((err > bound[written]).sum()), err.size, worst)


def run_alone(name, p, c0):
    """The case as its own tnr_sgemm call, twice; -> the destination's bits (judged)."""
    L = Loaded(p)
    runs = []
    for _ in range(2):
        c, part = L.fresh(c0)
        sgemm(L.fields(c, part))
        runs.append((c, part))
    torch.cuda.synchronize()
    got = [bits(c) for c, _ in runs]
    assert np.array_equal(got[0], got[1]), "%s: two runs differ" % name
    for _, part in runs:
        L.check_part(name, part)
    judge(name, got[0], c0, R.apply(c0, p))
    return got[0]


# ------------------------------------------------------------------------------------------------ (a) - (d): every table entry
@pytest.mark.parametrize("name", R.CASES)
def test_sgemm_against_float64(name):
    p, c0 = R.case(name)
    run_alone(name, p, c0)


def test_fallback_to_one_slice_leaves_the_partial_buffer():
    """K = 16 asked for 8 slices: one slice is left, the partial buffer that still has to be passed is not touched."""
    for name in ("split/dW_K16_ks8_batch3", "split/kfast_K16_ks8_batch1"):
        p, c0 = R.case(name)
        L = Loaded(p)
        assert L.pe == 0 and p["beta"] == 1.0
        c, part = L.fresh(c0)
        sgemm(L.fields(c, part))
        torch.cuda.synchronize()
        assert part.numel() == GUARD and (part == SENT).all()
        judge(name, bits(c), c0, R.apply(c0, p))


# ------------------------------------------------------------------------------------------------ (e) a row's bits and its company
@pytest.mark.parametrize("K,ksplit", [(65, 1), (600, 8)])
def test_row_bits_do_not_depend_on_the_rows_around(K, ksplit):
    """The promise in-batch de-duplication and the frozen-layer cache rest on (Engine._sgemm_problem): a row of the
    k-fast forward form comes out with the same bits alone, in another tile position, or as a member of a batch."""
    M, N = 130, 70
    rs = np.random.RandomState(K)
    A, B, bias = (rs.standard_normal(s).astype(np.float32) for s in ((M, K), (N, K), (N,)))

    def call(a, b, bi, m, batch=1):
        p = dict(A=a.reshape(-1), a_off=0, a_rs=K, a_cs=1, sA=m * K, B=b.reshape(-1), b_off=0, b_rs=K, b_cs=1, sB=N * K, bias=bi.reshape(-1),
                 bias_off=0, sBias=N, M=m, N=N, K=K, batch=batch, alpha=1.0, beta=0.0, ksplit=ksplit, ldc=N, sC=m * N)
        c0 = R.destination(p, rs, "sent")
        got = run_alone("rows K%d ksplit%d M%d batch%d" % (K, ksplit, m, batch), p, c0)
        return got[GUARD:len(got) - GUARD].reshape(batch, m, N)

    full = call(A, B, bias, M)[0]
    for r0, m in ((129, 1), (3, 64), (64, 65)):
        part = call(A[r0:r0 + m], B, bias, m)[0]
        assert np.array_equal(part, full[r0:r0 + m]), "rows %d..%d differ from the full call's" % (r0, r0 + m - 1)
    other = lambda x: rs.standard_normal((2,) + x.shape).astype(np.float32)
    member = call(np.concatenate([other(A), A[None]]), np.concatenate([other(B), B[None]]), np.concatenate([other(bias), bias[None]]), M, 3)
    assert np.array_equal(member[2], full), "member 2 of a batch of 3 differs from the call of its own"
    assert not np.array_equal(member[0], full)


# ------------------------------------------------------------------------------------------------ (f) groups
def run_group(gname):
    names = R.GROUPS[gname]
    cases = [R.case(n) for n in names]
    loaded = [Loaded(p) for p, _ in cases]
    runs = []
    for _ in range(2):
        bufs = [L.fresh(c0) for L, (_, c0) in zip(loaded, cases)]
        T.sgemm_group([L.fields(c, part) for L, (c, part) in zip(loaded, bufs)])
        runs.append(bufs)
    alone = [L.fresh(c0) for L, (_, c0) in zip(loaded, cases)]
    for L, (c, part) in zip(loaded, alone):
        sgemm(L.fields(c, part))
    torch.cuda.synchronize()
    for i, (n, L, (p, c0)) in enumerate(zip(names, loaded, cases)):
        what = "group %s[%d] %s" % (gname, i, n)
        got = bits(runs[0][i][0])
        assert np.array_equal(got, bits(runs[1][i][0])), "%s: two runs differ" % what
        L.check_part(what, runs[0][i][1])
        L.check_part(what, runs[1][i][1])
        judge(what, got, c0, R.apply(c0, p))
        assert np.array_equal(got, bits(alone[i][0])), "%s: differs from its own tnr_sgemm call" % what
    return loaded


@pytest.mark.parametrize("gname", sorted(R.GROUPS))
def test_group_members_against_float64_and_their_own_calls(gname):
    loaded = run_group(gname)
    if gname == "fallback":        # the only member that asked for a split has one slice: nothing for a reduce launch to do
        assert [L.pe for L in loaded] == [0, 0, 0] and loaded[1].p["ksplit"] == 8 and loaded[1].p["beta"] == 1.0


def _refused(call, dests, where):
    before = [bits(c) for c in dests]
    with pytest.raises(T.TnrError):
        call()
    torch.cuda.synchronize()
    msg = T.lib().tnr_last_error().decode()
    assert msg and where in msg, msg
    for c, b in zip(dests, before):
        assert np.array_equal(bits(c), b), "a refused call changed its destination"
    return msg


@pytest.mark.parametrize("n", [0, 9])
def test_group_refuses_no_problem_and_nine(n):
    p, c0 = R.case("edge/M33_N65_K65")
    L = Loaded(p)
    dests = [dev(c0) for _ in range(n)]
    _refused(lambda: T.sgemm_group([L.fields(c, None) for c in dests]), dests, "tnr_sgemm_group")


def test_group_refuses_a_bad_member_and_writes_nothing():
    """A group with a refused member launches nothing: the good members' destinations keep their bits too."""
    p, c0 = R.case("edge/M33_N65_K65")
    L = Loaded(p)
    dests = [dev(c0), dev(c0)]
    for bad in (dict(K=0), dict(B=None), dict(ksplit=2, part=None)):
        _refused(lambda: T.sgemm_group([L.fields(dests[0], None), dict(L.fields(dests[1], None), **bad)]), dests, "tnr_sgemm_group")


# ------------------------------------------------------------------------------------------------ (g) refusals of tnr_sgemm
REFUSALS = [("A_null", dict(A=None)), ("B_null", dict(B=None)), ("C_null", dict(C=None)), ("M0", dict(M=0)), ("N0", dict(N=0)),
            ("K0", dict(K=0)), ("batch0", dict(batch=0)), ("a_idx", dict(a_idx=True)), ("split_without_part", dict(ksplit=2, part=None))]


@pytest.mark.parametrize("what,bad", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_sgemm_refuses(what, bad):
    p, c0 = R.case("edge/M33_N65_K65")
    assert p["K"] >= 17
    L = Loaded(p)
    c = dev(c0)
    q = dict(L.fields(c, None), **{k: v for k, v in bad.items() if k != "a_idx"})
    idx = torch.zeros(p["M"], dtype=torch.int32, device=DEV) if "a_idx" in bad else None

    def call():
        T.call("tnr_sgemm", q["A"], q["a_rs"], q["a_cs"], q["sA"], idx, q["B"], q["b_rs"], q["b_cs"], q["sB"], q["C"], q["ldc"], q["sC"],
               q["bias"], q["sBias"], q["M"], q["N"], q["K"], q["batch"], q["alpha"], q["beta"], q["ksplit"], q["part"])
    _refused(call, [c], "tnr_sgemm")
