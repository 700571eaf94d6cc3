"""tnr_lamb_norms / tnr_lamb_commit / tnr_lamb_step (csrc/lamb.hip) through the C ABI on a synthetic slot table, against the float64
reference of tests/lamb_ref.py.  No engine: engine.lamb_chunks (a pure host function) makes the chunk table.

The table: tensors of 1, 3, 4, 5, 255, 4095, 4096, 4097 and 2 x 4096 + 1 elements, each size starting at an element offset of
0, 1, 2 and 3 modulo 4, with gaps of 0 .. 63 elements between them; three in four are 2-D `.weight`s (adapted), the rest biases;
plus a zero matrix and a matrix / bias pair with zero gradient and zero moments.  Every buffer holds NaN in its gap elements and
in 64 elements in front of and behind it; the partial and trust tables have NaN behind them.  All of those must keep their bits
and none may reach a norm.

Bounds: trust, ||w||, ||u||: lamb_ref.trust_rtol / norm_rtol, derived from the kernel's summation order and the roundings of u
(tests/lamb_ref.py); p rtol 1e-5 atol 1e-6; m, v, vmax rtol 1e-5 with a floor of 1e-5 of the buffer's largest magnitude (the
bounds of tests/test_adamw_kernels_gpu.py); the average as p."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import lamb_ref as L                                    # noqa: E402
import tnr_hip as T                                     # noqa: E402
from test_heads_kernels_gpu import check, check_abs     # noqa: E402

DEV = "cuda:0"
FRONT = BACK = 64
SIZES = [1, 3, 4, 5, 255, 4095, 4096, 4097, 2 * 4096 + 1]
B1, B2, EPS, GS, WD = (L.f32(x) for x in (0.9, 0.999, 1e-8, 0.5, 0.01))
LRS = tuple(L.f32(x) for x in (2e-2, 1.3e-2, 7e-3))
EMW = tuple(L.f32(x) for x in (0.1, 0.25, 0.5))
_C = {}


def layout():
    """-> dict(table, n, names, chunks, tensors, covered): the synthetic slot table and its chunk table."""
    if "lay" not in _C:
        import engine as E
        table, o, i = [], 0, 0
        for r in range(4):
            for k in SIZES:
                gap = (7 * i) % 16 * 4                   # 0 .. 60, then up to + 3 to reach the offset's residue: gaps of 0 .. 63
                o += gap
                o += (r - o) % 4
                adapted = i % 4 != 3
                table.append(("t%d.%s" % (i, "weight" if adapted else "bias"), o, k, (k, 1) if adapted else (k,)))
                o += k
                i += 1
        for name, shp in (("zero.weight", (37, 3)), ("still.weight", (29, 5)), ("still.bias", (131,))):
            o += 5
            table.append((name, o, int(np.prod(shp)), shp))
            o += int(np.prod(shp))
        n = (o + 63) // 64 * 64
        slot = {name: (True, off, k, shp) for name, off, k, shp in table}
        names, chunks, tensors = E.lamb_chunks(slot, n)
        L.check_chunks(table, n, chunks, tensors, names)
        covered = np.zeros(n, bool)
        for _, off, k, _ in table:
            covered[off:off + k] = True
        order = sorted(table, key=lambda e: e[1])
        gaps = [b[1] - (a[1] + a[2]) for a, b in zip(order, order[1:])]
        assert min(gaps) == 0 and 48 <= max(gaps) <= 63
        assert {(e[1] % 4, e[2]) for e in table} >= {(r, k) for r in range(4) for k in SIZES}
        _C["lay"] = dict(table=table, n=n, names=names, chunks=chunks, tensors=tensors, covered=covered,
                         by={e[0]: e for e in table})
    return _C["lay"]


def inputs():
    """p, g, m, v, vmax, ema in mid-training (m of either sign, v > 0, vmax >= v), NaN in every gap element; never modified."""
    if "in" not in _C:
        lay = layout()
        n, rs = lay["n"], np.random.RandomState(17)
        p, g, m = rs.standard_normal(n) * 0.05, rs.standard_normal(n) * 0.1, rs.standard_normal(n) * 0.05
        v = np.abs(rs.standard_normal(n)) * 0.01
        x = v + np.abs(rs.standard_normal(n)) * 0.01 * (rs.rand(n) < 0.5)
        e = p + rs.standard_normal(n) * 0.01
        sl = lambda name: slice(lay["by"][name][1], lay["by"][name][1] + lay["by"][name][2])
        p[sl("zero.weight")] = 0.0
        for name in ("still.weight", "still.bias"):
            for b in (g, m, v, x):
                b[sl(name)] = 0.0
        bufs = [b.astype(np.float32) for b in (p, g, m, v, x, e)]
        for b in bufs:
            b[~lay["covered"]] = np.nan
        _C["in"] = bufs
    return _C["in"]


class Flat:
    """A flat device buffer with FRONT / BACK NaN elements around it (FRONT keeps the 16-byte alignment)."""

    def __init__(self, fill):
        n = len(fill)
        self.raw = torch.full((FRONT + n + BACK,), float("nan"), device=DEV, dtype=torch.float32)
        self.t = self.raw[FRONT:FRONT + n]
        self.t.copy_(torch.from_numpy(fill))
        self.start = self.raw.clone()

    def bits(self):
        return self.raw.view(torch.int32)

    def outside_ok(self, covered_dev):
        a, b = self.bits(), self.start.view(torch.int32)
        n = self.t.numel()
        return bool(torch.equal(a[:FRONT], b[:FRONT]) and torch.equal(a[FRONT + n:], b[FRONT + n:]) and
                    torch.equal(a[FRONT:FRONT + n][~covered_dev], b[FRONT:FRONT + n][~covered_dev]))


def tables():
    if "tab" not in _C:
        lay = layout()
        ch, tn = torch.from_numpy(lay["chunks"]).contiguous(), torch.from_numpy(lay["tensors"]).contiguous()
        _C["tab"] = dict(ch=ch, tn=tn, chd=ch.to(DEV), tnd=tn.to(DEV), nc=len(ch), nt=len(tn), cov=torch.from_numpy(lay["covered"]).to(DEV))
    return _C["tab"]


def run(ams, ema, wd=WD, clip=None, guard=None, stamp=0, known=0, step=3, split=None):
    """The three launches on fresh buffers -> dict of Flat (p, g, m, v, x, e, part, trust)."""
    tb = tables()
    p, g, m, v, x, e = (Flat(b) for b in inputs())
    part = Flat(np.full(2 * tb["nc"], -3.0, np.float32))
    trust = Flat(np.full(3 * tb["nt"], -3.0, np.float32))
    n = p.t.numel()
    vm, em = (x.t if ams else None), (e.t if ema else None)
    T.call("tnr_lamb_norms", p.t, g.t, m.t, v.t, vm, n, tb["chd"], tb["ch"], tb["nc"], tb["nt"], step, B1, B2, EPS, GS, wd, guard,
           stamp, known, clip, part.t)
    T.call("tnr_lamb_commit", part.t, tb["nc"], tb["tnd"], tb["tn"], tb["nt"], trust.t, guard, stamp)
    for c0, c1 in ([(0, tb["nc"])] if split is None else [(0, split), (split, tb["nc"])]):
        T.call("tnr_lamb_step", p.t, g.t, m.t, v.t, vm, n, tb["chd"][c0:c1], tb["ch"][c0:c1], c1 - c0, tb["nt"], step, LRS[0], LRS[1],
               LRS[2], B1, B2, EPS, GS, wd, guard, stamp, known, clip, trust.t, em, EMW[0], EMW[1], EMW[2])
    return dict(p=p, g=g, m=m, v=v, x=x, e=e, part=part, trust=trust)


def run_twice(*a, **kw):
    one, two = run(*a, **kw), run(*a, **kw)
    torch.cuda.synchronize()
    cov = tables()["cov"]
    for k in one:
        assert torch.equal(one[k].bits(), two[k].bits()), "%s: two runs differ" % k
        if k in ("part", "trust"):
            assert one[k].outside_ok(torch.ones_like(one[k].t, dtype=torch.bool)), "%s: wrote outside its table" % k
        else:
            assert one[k].outside_ok(cov), "%s: a gap or sentinel element changed" % k
    assert torch.equal(one["g"].bits(), one["g"].start.view(torch.int32))
    return one


def reference(ams, ema, wd, coef, k=0, step=3):
    lay = layout()
    p, g, m, v, x, e = (b.astype(np.float64) for b in inputs())
    out = L.lamb_step(lay["table"], p, g, m, v, x if ams else None, step - k, LRS[k], wd, B1, B2, EPS, grad_scale=GS * coef)
    e2 = e + EMW[k] * (out[0] - e) if ema else None
    return dict(p=out[0], m=out[1], v=out[2], x=out[3], e=e2, info=out[4])


def compare(what, got, want, ams, ema):
    lay, tb = layout(), tables()
    cov = lay["covered"]
    h = lambda f: f.t.cpu().numpy().astype(np.float64)
    check_abs("%s/p" % what, h(got["p"])[cov], want["p"][cov], 1e-5, 1e-6)
    check("%s/m" % what, h(got["m"])[cov], want["m"][cov], 1e-5, 1e-5)
    check("%s/v" % what, h(got["v"])[cov], want["v"][cov], 1e-5, 1e-5)
    if ams:
        check("%s/vmax" % what, h(got["x"])[cov], want["x"][cov], 1e-5, 1e-5)
    else:
        assert torch.equal(got["x"].bits(), got["x"].start.view(torch.int32))
    if ema:
        check_abs("%s/ema" % what, h(got["e"])[cov], want["e"][cov], 1e-5, 1e-6)
    else:
        assert torch.equal(got["e"].bits(), got["e"].start.view(torch.int32))
    tr = h(got["trust"])
    nt, worst = tb["nt"], 0.0
    for t, name in enumerate(lay["names"]):
        trust, wn, un, kappa = want["info"][name]
        if not lay["tensors"][t, 2]:
            assert (tr[t], tr[nt + t], tr[2 * nt + t]) == (1.0, 0.0, 0.0), name
            continue
        bound = L.trust_rtol(kappa)
        assert bound < 1e-5, (name, kappa, bound)
        assert np.isfinite(tr[t]) and abs(tr[t] - trust) <= bound * abs(trust), (what, name, tr[t], trust, bound)
        assert abs(tr[nt + t] - wn) <= L.norm_rtol(1.0, of_u=False) * wn, (what, name, "w norm")
        assert abs(tr[2 * nt + t] - un) <= L.norm_rtol(kappa) * un, (what, name, "u norm")
        if trust != 0.0:
            worst = max(worst, abs(tr[t] - trust) / (bound * abs(trust)))
    print("[lamb-kernels] %s: worst trust err / bound %.3f" % (what, worst))
    return tr


@pytest.mark.parametrize("ema", [0, 1])
@pytest.mark.parametrize("ams", [1, 0])
def test_sizes_offsets_and_gaps_against_float64(ams, ema):
    """Every size at every offset modulo 4, with and without a clip coefficient read from the device, wd = 0.01 and 0."""
    lay = layout()
    half = torch.tensor([0.5, 123.0], dtype=torch.float32, device=DEV)
    for wd in (WD, 0.0):
        for clip in (None, half):
            got = run_twice(ams, ema, wd=wd, clip=clip)
            want = reference(ams, ema, wd, 0.5 if clip is not None else 1.0)
            tr = compare("lamb ams%d ema%d wd%g clip%d" % (ams, ema, wd, clip is not None), got, want, ams, ema)
            t = {name: tr[i] for i, name in enumerate(lay["names"])}
            assert t["zero.weight"] == 1.0 and t["still.bias"] == 1.0                  # a zero tensor; an exempt tensor
            if wd == 0.0:
                assert t["still.weight"] == 1.0                                         # a zero update divides nothing
            else:
                assert abs(t["still.weight"] - 1.0 / wd) <= L.trust_rtol(1.0) / wd      # u = wd w
            adapted = [tr[i] for i in range(len(lay["names"])) if lay["tensors"][i, 2]]
            assert np.isfinite(adapted).all() and sum(abs(a - 1.0) > 0.1 for a in adapted) > len(adapted) // 2     # the ratio shows
    # the zero tensor leaves zero with trust 1; the still pair moves only through the coupled decay
    z = lay["by"]["zero.weight"]
    assert float(got["p"].t[z[1]:z[1] + z[2]].abs().min()) > 0.0


def test_two_launches_over_parts_of_the_table_are_one():
    """tnr_lamb_step over chunks [0, c) and [c, n_chunks) (a rate range each, as Engine.step launches them): the bits of one launch."""
    a = run_twice(1, 1)
    b = run_twice(1, 1, split=tables()["nc"] // 3)
    for k in a:
        assert torch.equal(a[k].bits(), b[k].bits()), k


@pytest.mark.parametrize("ams", [1, 0])
def test_guard_picks_one_candidate_in_both_passes(ams):
    """guard[1] - known_skips = 0, 1, 2, 3 -> the bias corrections, rate and average weight of candidates 0, 1, 2, 2 in the norm pass
    AND the apply pass: step 5, so c1 = 1 - 0.9^t differs by 19 % and 27 % between neighbours, and a norm pass on another candidate
    than the apply pass would miss trust by that much.  guard[0] == stamp: no bit of anything changes, the tables included."""
    seen = []
    for k in (0, 1, 2, 3):
        guard = torch.tensor([3, 4 + k, 0, 0], dtype=torch.int32, device=DEV)
        got = run_twice(ams, 1, guard=guard, stamp=7, known=4, step=5)
        want = reference(ams, 1, WD, 1.0, k=min(k, 2), step=5)
        seen.append(compare("lamb guard k%d ams%d" % (k, ams), got, want, ams, 1))
        assert guard.tolist() == [3, 4 + k, 0, 0]
    ad = [t for t in range(tables()["nt"]) if layout()["tensors"][t, 2]]
    seen = [s_[ad] for s_ in seen]
    assert np.abs(seen[0] / seen[1] - 1.0).max() > 0.05 and np.abs(seen[1] / seen[2] - 1.0).max() > 0.05 and (seen[2] == seen[3]).all()
    guard = torch.tensor([9, 1, 0, 0], dtype=torch.int32, device=DEV)
    half = torch.tensor([0.5, 1.0], dtype=torch.float32, device=DEV)
    got = run_twice(ams, 1, guard=guard, stamp=9, known=0, step=5, clip=half)
    for k in got:
        assert torch.equal(got[k].bits(), got[k].start.view(torch.int32)), k


def test_bad_arguments_are_errors_not_launches():
    tb = tables()
    p, g, m, v, x, e = (Flat(b) for b in inputs())
    part = Flat(np.full(2 * tb["nc"], -3.0, np.float32))
    trust = Flat(np.full(3 * tb["nt"], 1.0, np.float32))
    n, nc, nt = p.t.numel(), tb["nc"], tb["nt"]
    everything = (p, g, m, v, x, e, part, trust)

    def bad(rows):
        c = tb["ch"].clone()
        for j, col, val in rows:
            c[j, col] = val
        return c
    beyond = bad([(nc - 1, 0, n - 1), (nc - 1, 1, 2)])
    norms = lambda **kw: [kw.get("p", p.t), g.t, m.t, v.t, x.t, kw.get("n", n), kw.get("chd", tb["chd"]), kw.get("ch", tb["ch"]),
                          kw.get("nc", nc), kw.get("nt", nt), kw.get("step", 3), B1, B2, EPS, GS, kw.get("wd", WD), None, 0, 0, None,
                          kw.get("part", part.t)]
    step = lambda **kw: norms(**kw)[:-1] + [kw.get("trust", trust.t), kw.get("ema", e.t), kw.get("w0", 0.1), 0.1, 0.1]
    step_args = lambda **kw: (lambda a: a[:10] + [a[10], LRS[0], LRS[1], LRS[2]] + a[11:])(step(**kw))
    cases = [("a NULL p", dict(p=None)), ("a NULL device table", dict(chd=None)), ("a NULL host table", dict(ch=None)),
             ("n_chunks 0", dict(nc=0)), ("n_chunks -1", dict(nc=-1)), ("n_tensors 0", dict(nt=0)), ("step 0", dict(step=0)),
             ("a chunk beyond n", dict(ch=beyond)), ("a chunk of 4097", dict(ch=bad([(0, 1, 4097)]))),
             ("a chunk of 0", dict(ch=bad([(0, 1, 0)]))), ("a negative first", dict(ch=bad([(0, 0, -4)]))),
             ("a tensor id past the table", dict(ch=bad([(5, 2, nt)]))), ("n below the last chunk", dict(n=n - 64 * 40)),
             ("weight_decay < 0", dict(wd=-0.1)), ("a misaligned p", dict(p=p.raw[FRONT + 1:FRONT + 1 + n]))]
    for what, kw in cases:
        with pytest.raises(T.TnrError):
            T.call("tnr_lamb_norms", *norms(**kw))
        with pytest.raises(T.TnrError):
            T.call("tnr_lamb_step", *step_args(**kw))
    for what, kw in (("a NULL part", dict(part=None)),):
        with pytest.raises(T.TnrError):
            T.call("tnr_lamb_norms", *norms(**kw))
    for what, kw in (("a NULL trust", dict(trust=None)), ("an average's weight above 1", dict(w0=1.5)),
                     ("a misaligned average", dict(ema=e.raw[FRONT + 1:FRONT + 1 + n]))):
        with pytest.raises(T.TnrError):
            T.call("tnr_lamb_step", *step_args(**kw))
    tn_bad = tb["tn"].clone()
    tn_bad[nt - 1, 1] += 1
    for args in ((None, nc, tb["tnd"], tb["tn"], nt, trust.t, None, 0), (part.t, nc, None, tb["tn"], nt, trust.t, None, 0),
                 (part.t, nc, tb["tnd"], None, nt, trust.t, None, 0), (part.t, nc, tb["tnd"], tb["tn"], nt, None, None, 0),
                 (part.t, 0, tb["tnd"], tb["tn"], nt, trust.t, None, 0), (part.t, nc, tb["tnd"], tb["tn"], 0, trust.t, None, 0),
                 (part.t, nc, tb["tnd"], tn_bad, nt, trust.t, None, 0), (part.t, nc - 1, tb["tnd"], tb["tn"], nt, trust.t, None, 0)):
        with pytest.raises(T.TnrError):
            T.call("tnr_lamb_commit", *args)
    torch.cuda.synchronize()
    for b in everything:
        assert torch.equal(b.bits(), b.start.view(torch.int32))
    assert "tnr_lamb" in T.lib().tnr_last_error().decode()
