"""The HBM-bound row kernels on the 16-bit activations (csrc/norm_embed.hip, csrc/attpool.hip with its fp32 stages in heads.hip,
tnr_relpos_table), one by one and in both builds, against the float64 references of tests/rows_ref.py (tied to the oracle, and
their bounds shown to be satisfiable, by tests/test_rows_ref_cpu.py), at the smallest shapes that reach each path: all four
widths of the LayerNorm template, the row tail inside the 8 rows of a workgroup and inside and across the 32-row blocks of the
backward, its short / tall switch at M = 32768, the seven call forms of the backward, the token loops' tails, second turns and
64-token chunk edges of both attention-pooling forms, leading dimensions above the width, widths off every vector and block size.

Every output buffer has a sentinel region behind it that must come back untouched, gap columns of padded outputs keep their
sentinel, every call runs twice and must give equal bits, and whatever lies where a kernel must not read - rows behind M, gap
columns, e columns >= Q, table rows behind the last - holds NaN.  The bounds are those of tests/rows_ref.py's docstring; every
comparison prints its largest error and that error as a fraction of its bound (EXPERIMENTS.md item 63 records them)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import rows_ref as R                           # noqa: E402
import tnr_hip as T                            # noqa: E402
from oracle import dropout_oracle as DO        # noqa: E402

DEV = "cuda:0"
SENT = -7.25                                   # exact in fp32, bf16 and fp16
GUARD = 64
NAN = float("nan")
U23 = R.U23
COLSUM_PAD_ROWS = 2                            # rows of NaN behind the M rows of a column-sum input


def dev(x, dt=None):
    t = torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    return t.to(dt) if dt is not None else t


def dev32(x):
    return dev(np.asarray(x, np.float32))


def dev_rows(x, dt, nan_rows=R.NAN_ROWS):
    """x (M, C) on the device as dt, with nan_rows rows of NaN directly behind it."""
    x = np.asarray(x, np.float32)
    t = torch.full((x.shape[0] + nan_rows, x.shape[1]), NAN, device=DEV, dtype=dt)
    t[:x.shape[0]] = dev(x).to(dt)
    return t


def host(t):
    return t.float().cpu().numpy().astype(np.float64)


class Buf:
    """An output buffer of `shape` with GUARD sentinel elements behind it; SENT everywhere unless `fill` (numpy) is given."""

    def __init__(self, *shape, dtype=torch.float32, fill=None):
        n = int(np.prod(shape))
        self.raw = torch.full((n + GUARD,), SENT, device=DEV, dtype=dtype)
        self.t = self.raw[:n].view(*shape)
        if fill is not None:
            self.t.copy_(dev32(fill).view(*shape))

    def guard_ok(self):
        return bool((self.raw[self.t.numel():] == SENT).all())

    def bits(self):
        return self.t.view(torch.int16 if self.t.element_size() == 2 else torch.int32)


def twice(fn):
    """fn() -> {name: Buf}: run it twice, require untouched guards and equal bits -> ({name: float64 numpy}, {name: Buf})."""
    a = fn()
    b = fn()
    torch.cuda.synchronize()
    for n in a:
        assert a[n].guard_ok() and b[n].guard_ok(), "%s: wrote behind its buffer" % n
        assert torch.equal(a[n].bits(), b[n].bits()), "%s: two runs differ" % n
    return {n: host(a[n].t) for n in a}, a


def check(what, got, ref, bound):
    """|got - ref| <= bound element by element, printing the largest error and the worst error / bound."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    bound = np.broadcast_to(np.asarray(bound, np.float64), ref.shape)
    assert got.shape == ref.shape, what
    err = np.abs(got - ref)
    ratio = np.where(err == 0.0, 0.0, err / np.maximum(bound, 1e-300))
    worst = float(ratio.max(initial=0.0))
    print("[rows-kernels] %s: max|err| %.3e, worst err / bound %.3f" % (what, float(err.max(initial=0.0)), worst))
    assert np.isfinite(got).all(), what + ": not finite"
    assert (err <= bound).all(), "%s: %d of %d elements over the bound, worst err / bound %.3f" % (what, int((err > bound).sum()), err.size, worst)


def check_fwd(what, got, ref):
    check(what, got, ref, R.FWD * np.abs(ref) + R.FLOOR * np.abs(ref).max(initial=0.0))


def same_bits(a, b):
    return torch.equal(a.bits(), b.bits())


# ------------------------------------------------------------------------------------------------ LayerNorm forward
@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("H", R.LN_H)
def test_ln_fwd(H, kind):
    """M on both sides of the 8 rows of a workgroup and of 32 and 64; rows of four kinds (rows_ref.ln_rows); NaN in the 8 rows
    behind M; stats = NULL gives the same y."""
    td, sfx = R.tdtype(kind), R.SFX[kind]
    for M in R.LN_M:
        c = R.ln_case(M, H, kind, False)
        f = R.ln_fwd(c["x"], c["g"], c["b"])
        x, g, b = dev_rows(c["x"], td), dev32(c["g"]), dev32(c["b"])

        def fn(stats=True):
            o = dict(y=Buf(M, H, dtype=td), stats=Buf(M, 2))
            T.call("tnr_ln_fwd" + sfx, x, g, b, R.EPS, o["y"].t, o["stats"].t if stats else None, M, H)
            return o
        got, bufs = twice(fn)
        tag = "M%d H%d %s" % (M, H, kind)
        check("ln_fwd/mean " + tag, got["stats"][:, 0], f["mean"], f["b_mean"])          # the statistics first: they are held to
        check("ln_fwd/rstd " + tag, got["stats"][:, 1], f["rstd"], f["b_rstd"])          # fp32 bounds, y to the 16-bit rounding
        check("ln_fwd/y " + tag, got["y"], f["y"], R.out16(f["y"], kind, f["fp_y"]))
        const = c["rk"] == 3                    # a constant row: y = the rounding of beta, mean = the value
        assert np.array_equal(got["y"][const], np.broadcast_to(R.r16(c["b"], kind), (int(const.sum()), H))), tag
        assert np.array_equal(got["stats"][const, 0], c["x"][const, 0]), tag
        got0, bufs0 = twice(lambda: fn(False))
        assert same_bits(bufs["y"], bufs0["y"]) and (got0["stats"] == SENT).all(), tag + ": stats = NULL"


# ------------------------------------------------------------------------------------------------ LayerNorm backward
def _ln_bwd_inputs(c, kind):
    td = R.tdtype(kind)
    f = R.ln_fwd(c["x"], c["g"], c["b"])
    st = R.ln_stats32(f)
    M = c["x"].shape[0]
    std = torch.full((M + R.NAN_ROWS, 2), NAN, device=DEV)
    std[:M] = dev(st)
    return st, (dev_rows(c["dy"], td), dev_rows(c["x"], td), std, dev32(c["g"]))


def _ln_bwd_run(sfx, td, inp, M, H, form, ws_elems, site=None):
    """form: "sums" dgamma, dbeta, dxsum in buffers of their own; "adjacent" dgamma and dbeta in one (the single-reduction
    branch); "part" all three NULL, partials only; "dgamma" / "dbeta" / "dxsum" only that one; "dx" part = NULL.  site: tnr_ln_bwd_do with dxm."""
    def fn():
        o = dict(dx=Buf(M, H, dtype=td))
        if form != "dx":
            o["part"] = Buf(ws_elems)
        if form == "sums":
            o.update(dgamma=Buf(H), dbeta=Buf(H), dxsum=Buf(H))
        elif form == "adjacent":
            o.update(dgdb=Buf(2 * H), dxsum=Buf(H))
        elif form in ("dgamma", "dbeta", "dxsum"):
            o[form] = Buf(H)
        p = lambda n: o[n].t if n in o else None
        dg, db = (o["dgdb"].t[:H], o["dgdb"].t[H:]) if form == "adjacent" else (p("dgamma"), p("dbeta"))
        if site is None:
            T.call("tnr_ln_bwd" + sfx, *inp, o["dx"].t, dg, db, p("dxsum"), p("part"), M, H)
        else:
            o["dxm"] = Buf(M, H, dtype=td)
            T.call("tnr_ln_bwd_do" + sfx, *inp, o["dx"].t, dg, db, p("dxsum"), p("part"), M, H, o["dxm"].t, site)
        return o
    got, bufs = twice(fn)
    if "dgdb" in got:
        got["dgamma"], got["dbeta"] = got["dgdb"][:H], got["dgdb"][H:]
    return got, bufs


def _ln_bwd_check(tag, kind, got, b, M, H, form, second="dx"):
    """`second`: the output whose rounded column sums dxsum holds (dx, or dxm under a site)."""
    check("ln_bwd/dx " + tag, got["dx"], b["dx"], R.out16(b["dx"], kind, b["fp_dx"]))
    nblk = T.query("tnr_ln_bwd_blocks", M)
    if form == "part":           # exactly nblk rows of [dgamma | dbeta | dxsum] partials, the rest of the workspace untouched
        part = got["part"]
        assert (part[nblk * 3 * H:] == SENT).all(), tag + ": more than tnr_ln_bwd_blocks(M) partial rows written"
        rows = part[:nblk * 3 * H].reshape(nblk, 3, H)
        # (a sum of 16-bit values can be the sentinel's value by accident: every section of every row holds something else)
        assert (rows != SENT).any(-1).all(), tag + ": fewer than tnr_ln_bwd_blocks(M) partial rows written"
        got = dict(got, dgamma=rows[:, 0].sum(0), dbeta=rows[:, 1].sum(0), dxsum=rows[:, 2].sum(0))
    if "dgamma" in got:
        check("ln_bwd/dgamma " + tag, got["dgamma"], b["dgamma"], b["b_dgamma"])
    if "dbeta" in got:
        check("ln_bwd/dbeta " + tag, got["dbeta"], b["dbeta"], b["b_dbeta"])
    if "dxsum" in got:           # the column sums of the ROUNDED output the kernel wrote; and, more loosely, the reference's
        check("ln_bwd/dxsum " + tag, got["dxsum"], got[second].sum(0), R.colsum_bound(got[second], b["count"]))
        check("ln_bwd/dxsum (reference) " + tag, got["dxsum"], b["dxsum"], b["b_dxsum"])


LN_FORMS = ("sums", "adjacent", "part", "dgamma", "dbeta", "dxsum", "dx")


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("H", R.LN_H)
def test_ln_bwd_call_forms(H, kind):
    """The row tails of the 8 rows of a turn and of the 32-row blocks (M = 33, 65: a second and third block), NaN in the 8 rows
    behind M of x, dy and stats, in the seven call forms; dx is the same bits in all seven."""
    td, sfx = R.tdtype(kind), R.SFX[kind]
    ws = T.query("tnr_ln_bwd_part_elems", max(R.LN_M), H)
    for M in R.LN_M:
        assert T.query("tnr_ln_bwd_blocks", M) == (M + 31) // 32
        c = R.ln_case(M, H, kind, True)
        st, inp = _ln_bwd_inputs(c, kind)
        b = R.ln_bwd(c["dy"], c["x"], st[:, 0], st[:, 1], c["g"], kind)
        first = None
        for form in LN_FORMS:
            got, bufs = _ln_bwd_run(sfx, td, inp, M, H, form, ws)
            _ln_bwd_check("%s M%d H%d %s" % (form, M, H, kind), kind, got, b, M, H, form)
            first = first or bufs
            assert same_bits(first["dx"], bufs["dx"]), "dx differs between call forms"


@pytest.mark.parametrize("kind", R.KINDS)
def test_ln_bwd_tall(kind):
    """H = 256 on both sides of the short / tall switch (32-row blocks below M = 32768, 128-row blocks from there on) and with a
    ragged last 128-row block; one workspace sized for M = 32777 serves all three."""
    td, sfx, H = R.tdtype(kind), R.SFX[kind], 256
    full = R.ln_case(R.LN_TALL[-1], H, kind, True)
    ws = T.query("tnr_ln_bwd_part_elems", R.LN_TALL[-1], H)
    assert ws == 1024 * 3 * H
    for M in R.LN_TALL:
        assert T.query("tnr_ln_bwd_blocks", M) == ((M + 31) // 32 if M < 32768 else (M + 127) // 128)
        c = dict(full, x=full["x"][:M], dy=full["dy"][:M])
        st, inp = _ln_bwd_inputs(c, kind)
        b = R.ln_bwd(c["dy"], c["x"], st[:, 0], st[:, 1], c["g"], kind)
        for form in ("sums", "part"):
            got, _ = _ln_bwd_run(sfx, td, inp, M, H, form, ws)
            _ln_bwd_check("%s M%d H%d %s" % (form, M, H, kind), kind, got, b, M, H, form)


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("H,M", R.LN_DO)
def test_ln_bwd_do_masked_second_output(H, M, kind):
    """An active site (p = 0.1, mask from oracle/dropout_oracle.py): dx the bits of the eval call, dxm the rounding of the UNROUNDED
    dx times mask / (1 - p), dxsum the column sums of dxm."""
    td, sfx = R.tdtype(kind), R.SFX[kind]
    p, seed, layer, call = 0.1, 0x1234567890ABCDEF, 2, 5
    m = DO.rows_mask(p, seed, DO.site_id(DO.KIND_FFN_OUT, layer), call, M, H)
    site = T.Dropout.site_of(p, seed, T.DROP_FFN_OUT, layer, call)
    c = R.ln_case(M, H, kind, True)
    st, inp = _ln_bwd_inputs(c, kind)
    b = R.ln_bwd(c["dy"], c["x"], st[:, 0], st[:, 1], c["g"], kind, mask=m)
    ws = T.query("tnr_ln_bwd_part_elems", M, H)
    _, ev = _ln_bwd_run(sfx, td, inp, M, H, "sums", ws)
    got, bufs = _ln_bwd_run(sfx, td, inp, M, H, "sums", ws, site=site)
    tag = "do M%d H%d %s" % (M, H, kind)
    assert same_bits(ev["dx"], bufs["dx"]), tag + ": dx differs from the eval call"
    _ln_bwd_check(tag, kind, got, b, M, H, "sums", second="dxm")
    check("ln_bwd/dxm " + tag, got["dxm"], b["dxm"], R.out16(b["dxm"], kind, b["fp_dxm"]))
    assert (m == 0).any() and (got["dxm"][m == 0] == 0).all()


# ------------------------------------------------------------------------------------------------ embedding + LayerNorm + mask
@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("H", R.LN_H)
def test_embed_ln_fwd_plain_and_indexed(H, kind):
    """n_tok = 1, 21, 64, 66, 512 (off and on the 4 tokens of a workgroup); L = 32: no pad columns, L = 33: 31 of them, L = 512: the
    last position row; a NaN row directly behind `word` and in the position rows >= L."""
    td, sfx = R.tdtype(kind), R.SFX[kind]
    for N, L in R.EMBED_NL:
        c = R.embed_case(N, L, H)
        Lr = R.ceil32(L)
        f = R.embed_ln(c["ids"], c["word"], c["pos"], c["type0"], c["g"], c["b"])
        par = [dev32(c[k]) for k in ("word", "pos", "type0", "g", "b")]

        def plain(ids, mask):
            tok = dev(np.concatenate([ids, mask], 1).astype(np.int64))

            def fn():
                o = dict(out=Buf(N * L, H, dtype=td), madd=Buf(N, Lr))
                T.call("tnr_embed_ln_fwd" + sfx, tok, N, L, H, *par, R.EPS, o["out"].t, o["madd"].t)
                return o
            return twice(fn)

        def madd_ok(ma, mask):
            assert np.array_equal(ma[:, :L], R.mask_add(mask)) and (ma[:, L:] <= -1e29).all(), tag + ": mask_add"
        tag = "N%d L%d H%d %s" % (N, L, H, kind)
        got, _ = plain(c["ids"], c["mask"])
        check("embed_ln/out " + tag, got["out"], f["y"], R.out16(f["y"], kind, f["fp_y"]))
        madd_ok(got["madd"], c["mask"])
        # indexed: an int32 table, nidx with repeats and the table's last row -> the bits of the plain form on the gathered rows
        tab, nidx = dev(c["table"]), dev(c["nidx"])

        def indexed():
            o = dict(out=Buf(N * L, H, dtype=td), madd=Buf(N, Lr))
            T.call("tnr_embed_ln_fwd_indexed" + sfx, tab, nidx, N, L, H, *par, R.EPS, o["out"].t, o["madd"].t)
            return o
        goti, bi = twice(indexed)
        rows = c["table"][c["nidx"]]
        gotg, bg = plain(rows[:, :L], rows[:, L:])
        assert same_bits(bi["out"], bg["out"]) and same_bits(bi["madd"], bg["madd"]), tag + ": indexed differs from plain"
        madd_ok(goti["madd"], rows[:, L:])
        fi = R.embed_ln(rows[:, :L], c["word"], c["pos"], c["type0"], c["g"], c["b"])
        check("embed_ln_indexed/out " + tag, goti["out"], fi["y"], R.out16(fi["y"], kind, fi["fp_y"]))


# ------------------------------------------------------------------------------------------------ cls / mean pooling
@pytest.mark.parametrize("mean", [0, 1])
@pytest.mark.parametrize("kind", R.KINDS)
def test_pool_fwd_bwd(kind, mean):
    """H = 4 (one thread), 1028 (a second turn of four columns); cls backward writes exact zeros to rows 1 .. L - 1."""
    td, sfx = R.tdtype(kind), R.SFX[kind]
    for H in R.POOL_H:
        for L in R.POOL_L:
            for n in R.POOL_N:
                y, dnv = R.pool_case(n, L, H, kind)
                yd, gd = dev_rows(y.reshape(n * L, H), td), dev_rows(dnv, torch.float32)
                tag = "n%d L%d H%d mean%d %s" % (n, L, H, mean, kind)
                got, _ = twice(lambda: _pool(sfx, "fwd", yd, Buf(n, H), n, L, H, mean))
                ref, bound = R.pool_fwd(y, mean)
                check("pool_fwd " + tag, got["out"], ref, bound)
                got, _ = twice(lambda: _pool(sfx, "bwd", gd, Buf(n * L, H, dtype=td), n, L, H, mean))
                ref, fp = R.pool_bwd(dnv, L, mean)
                check("pool_bwd " + tag, got["out"].reshape(n, L, H), ref, R.out16(ref, kind, fp))
                if not mean:
                    assert (got["out"].reshape(n, L, H)[:, 1:] == 0).all(), tag


def _pool(sfx, which, src, out, n, L, H, mean):
    T.call("tnr_pool_%s%s" % (which, sfx), src, out.t, n, L, H, mean)
    return dict(out=out)


# ------------------------------------------------------------------------------------------------ column sums
def _colsum(sfx, intype, M, N, ldx, acc, batch, gap, batched):
    """The matrices lie `sX = (M + COLSUM_PAD_ROWS) ldx + gap` apart in a buffer of NaN: gap columns, the rows behind M and the
    space between two matrices are NaN.  -> (got, reference, bound)."""
    x, o0 = R.colsum_case(M, N, intype, batch)
    rows = M + COLSUM_PAD_ROWS
    sX = rows * ldx + gap
    X = np.full((batch, sX), np.nan, np.float32)
    for z in range(batch):
        X[z, :rows * ldx].reshape(rows, ldx)[:M, :N] = x[z]
    Xd = dev(X, torch.float32 if intype == "f32" else R.tdtype(intype))
    code = {"f32": T.F32, "bf16": T.BF16, "f16": T.F16}[intype]
    pe = batch * T.query("tnr_colsum_part_elems", M, N)

    def fn():
        o = dict(out=Buf(batch, N, fill=o0 if acc else None), part=Buf(pe))
        if batched:
            T.call("tnr_colsum_batched" + sfx, Xd, ldx, sX, code, M, N, batch, o["out"].t, o["part"].t, acc)
        else:
            T.call("tnr_colsum" + sfx, Xd, ldx, code, M, N, o["out"].t, o["part"].t, acc)
        return o
    got, _ = twice(fn)
    ref, bound = R.colsum(x, o0 if acc else None)
    return got["out"], ref, bound


@pytest.mark.parametrize("intype", ["16", "f32"])
@pytest.mark.parametrize("kind", R.KINDS)
def test_colsum(kind, intype):
    """M on both sides of the 4 row lanes and of the 64-row blocks, M = 32773 (the 512-row blocks of tall inputs, a ragged last
    one); N off the 256 columns of a workgroup, a row of five workgroups and four columns; the 16-bit input of the build and fp32
    input through the same build's entry point."""
    it = kind if intype == "16" else "f32"
    for M, N in R.COLSUM_SHAPES:
        for ldx in (N, N + 12):
            for acc in (0, 1):
                got, ref, bound = _colsum(R.SFX[kind], it, M, N, ldx, acc, 1, 0, False)
                check("colsum M%d N%d ldx%d acc%d %s in %s" % (M, N, ldx, acc, kind, it), got, ref, bound)


@pytest.mark.parametrize("intype", ["16", "f32"])
@pytest.mark.parametrize("kind", R.KINDS)
def test_colsum_batched(kind, intype):
    it = kind if intype == "16" else "f32"
    for batch, M, N in R.COLSUM_BATCHED:
        for acc in (0, 1):
            got, ref, bound = _colsum(R.SFX[kind], it, M, N, N + 12, acc, batch, 8, True)
            check("colsum_batched b%d M%d N%d acc%d %s in %s" % (batch, M, N, acc, kind, it), got, ref, bound)


# ------------------------------------------------------------------------------------------------ additive-attention pooling
def _attpool(long, kind, L, H, Q, lde, lddpre):
    td, sfx, n = R.tdtype(kind), R.SFX[kind], R.AP_N
    Lr = R.ceil32(L)
    c = R.attpool_case(L, H, Q, kind)
    tag = "%s L%d H%d Q%d lde%d lddpre%d %s" % ("long" if long else "one", L, H, Q, lde, lddpre, kind)
    e = np.full((n * L, lde), np.nan, np.float32)          # the kernels read only q < Q
    e[:, :Q] = c["e"].reshape(n * L, Q)
    y, ed, w2, b2, dnv = dev_rows(c["y"].reshape(n * L, H), td), dev(e), dev32(c["w2"]), dev32([c["b2"]]), dev32(c["dnv"])
    ws_n = T.query("tnr_attpool_long_ws_elems" + sfx, n, L, H, Q, lddpre)

    def fwd():
        o = dict(nv=Buf(n, H), alpha=Buf(n, Lr), den=Buf(n))
        if long:
            o["ws"] = Buf(ws_n)
            T.call("tnr_attpool_fwd_long" + sfx, y, ed, lde, w2, b2, Q, o["nv"].t, o["alpha"].t, o["den"].t, o["ws"].t, n, L, H)
        else:
            T.call("tnr_attpool_fwd" + sfx, y, ed, lde, w2, b2, Q, o["nv"].t, o["alpha"].t, o["den"].t, n, L, H)
        return o
    got, _ = twice(fwd)
    f = R.attpool_fwd(c["y"], c["e"], c["w2"], c["b2"])
    check_fwd("attpool_fwd/nv " + tag, got["nv"], f["nv"])
    check_fwd("attpool_fwd/alpha " + tag, got["alpha"][:, :L], f["alpha"])
    check_fwd("attpool_fwd/den " + tag, got["den"], f["den"])
    assert (got["alpha"][:, L:] == 0).all(), tag + ": alpha columns L .. Lr"

    # backward from the reference's alpha as fp32 (zeros in the columns L .. Lr, as the forward leaves them)
    a32 = np.zeros((n, Lr), np.float32)
    a32[:, :L] = f["alpha"]
    al, den = dev(a32), dev32(f["den"])
    b = R.attpool_bwd(c["y"], c["e"], c["w2"], a32[:, :L], c["dnv"], kind)

    def bwd(db1=True):
        o = dict(dy=Buf(n * L, H, dtype=td), dpre=Buf(n * L, lddpre, dtype=td), dw2=Buf(n, Q), db2=Buf(n))
        if db1:
            o["db1"] = Buf(n, lddpre)
        p1 = o["db1"].t if db1 else None
        if long:
            o["ws"] = Buf(ws_n)
            T.call("tnr_attpool_bwd_long" + sfx, y, ed, lde, w2, Q, dnv, al, o["dy"].t, o["dpre"].t, lddpre, o["dw2"].t, o["db2"].t, p1,
                   o["ws"].t, n, L, H)
        else:
            T.call("tnr_attpool_bwd" + sfx, y, ed, lde, w2, Q, dnv, al, den, o["dy"].t, o["dpre"].t, lddpre, o["dw2"].t, o["db2"].t, p1,
                   n, L, H)
        return o
    got, bufs = twice(bwd)
    dpre = got["dpre"].reshape(n, L, lddpre)
    check("attpool_bwd/dy_direct " + tag, got["dy"].reshape(n, L, H), b["dy_direct"], R.out16(b["dy_direct"], kind, b["fp_dy_direct"]))
    check("attpool_bwd/dpre " + tag, dpre[..., :Q], b["dpre"], R.out16(b["dpre"], kind, b["fp_dpre"]))
    assert (dpre[..., Q:] == 0).all(), tag + ": dpre columns Q .. lddpre"
    check("attpool_bwd/dw2_part " + tag, got["dw2"], b["dw2_part"], b["b_dw2_part"])
    # a cancelling sum, held absolutely against its neighbour
    check("attpool_bwd/db2_part " + tag, got["db2"], b["db2_part"], R.DB2 * np.abs(b["dw2_part"]).max())
    # the per-sequence column sums of the ROUNDED dpre the kernel wrote: L terms
    check("attpool_bwd/db1_part " + tag, got["db1"], dpre.sum(1), L * U23 * np.abs(dpre).sum(1))
    check("attpool_bwd/db1_part (reference) " + tag, got["db1"][:, :Q], b["db1_part"], b["b_db1_part"])
    _, bufs0 = twice(lambda: bwd(False))
    for k in ("dy", "dpre", "dw2", "db2"):
        assert same_bits(bufs[k], bufs0[k]), tag + ": %s differs with db1_part = NULL" % k


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("long", [0, 1])
def test_attpool_real_shape_sweep_over_L(long, kind):
    """H = 768, Q = 200, lde = lddpre = 256, n = 3 (n_tok off 4).  One workgroup per sequence: the 4-wave token loop's tail
    (L = 1, 3, 5), L on both sides of 32 and of the 256-thread loops' second turn, 512.  Chunked: L on both sides of one, two and
    four 64-token chunks, 512."""
    for L, H, Q, lde, lddpre in R.attpool_cases(long)[:len(R.AP_L_LONG if long else R.AP_L_ONE)]:
        _attpool(long, kind, L, H, Q, lde, lddpre)


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("long", [0, 1])
def test_attpool_odd_widths(long, kind):
    """(H, Q, lde, lddpre) = (4, 1, 1, 1), (260, 64, 72, 64), (1028, 65, 208, 320) at L = 5 and 129: H off 1024 and 256, Q off 64,
    lde != lddpre on either side, a second turn of the lddpre loop."""
    for L, H, Q, lde, lddpre in R.attpool_cases(long)[len(R.AP_L_LONG if long else R.AP_L_ONE):]:
        _attpool(long, kind, L, H, Q, lde, lddpre)


# ------------------------------------------------------------------------------------------------ shadow copies
@pytest.mark.parametrize("mode", ["dst", "dstT", "both"])
@pytest.mark.parametrize("kind", R.KINDS)
def test_refresh_shadows(kind, mode):
    """One call with six descriptors; ld / ldT above the width with sentinels in the gaps and behind; every written element the
    bits of torch's CPU cast of the fp32 source (ties of both parities, -0.0, subnormals of the type, for fp16 values that round
    to infinity and one that just does not), everything else its sentinel."""
    td, sfx = R.tdtype(kind), R.SFX[kind]
    srcs = [R.shadow_source(r, c, kind, 10 + i) for i, (r, c) in enumerate(R.SHADOW_SHAPES)]
    sd = [dev(s) for s in srcs]
    sent = int(torch.tensor([SENT], dtype=td).view(torch.int16)[0])

    def fn():
        o, desc, start = {}, [], [0]
        for i, (r, c) in enumerate(R.SHADOW_SHAPES):
            ld, ldT = c + 3, r + 5
            d = Buf(r, ld, dtype=td) if mode != "dstT" else None
            dT = Buf(c, ldT, dtype=td) if mode != "dst" else None
            if d is not None:
                o["dst%d" % i] = d
            if dT is not None:
                o["dstT%d" % i] = dT
            desc.append([sd[i].data_ptr(), r, c, d.t.data_ptr() if d else 0, ld, dT.t.data_ptr() if dT else 0, ldT, 0])
            start.append(start[-1] + ((r + 31) // 32) * ((c + 31) // 32))
        dd, st = torch.tensor(desc, dtype=torch.int64, device=DEV), torch.tensor(start, dtype=torch.int64, device=DEV)
        T.call("tnr_refresh_shadows" + sfx, dd, len(desc), start[-1], st)
        torch.cuda.synchronize()                # the tables stay alive until the launch is done
        return o
    _, bufs = twice(fn)
    for i, (r, c) in enumerate(R.SHADOW_SHAPES):
        want = R.shadow_cast(srcs[i], kind)
        for name, w in (("dst%d" % i, want), ("dstT%d" % i, want.T)):
            if name in bufs:
                g = bufs[name].bits().cpu().numpy()
                assert np.array_equal(g[:, :w.shape[1]], w), "%s (%d, %d) %s: not the bits of the CPU cast" % (name, r, c, kind)
                assert (g[:, w.shape[1]:] == sent).all(), "%s (%d, %d) %s: wrote into the gap columns" % (name, r, c, kind)


# ------------------------------------------------------------------------------------------------ rel-pos table
@pytest.mark.parametrize("A", R.RELPOS_A)
def test_relpos_table(A):
    """L - 1 = 31, 32, 90, 91: a bucket edge as the largest distance and one past it; 512: every bucket; pad rows and columns 0."""
    w = np.random.RandomState(A).standard_normal((A, 32)).astype(np.float32)
    wd = dev(w)
    for L in R.RELPOS_L:
        Lr = R.ceil32(L)
        got, _ = twice(lambda: _relpos(wd, A, L, Lr))
        t = got["table"]
        assert np.array_equal(t[:, :L, :L], R.relpos_table(w, L)), "A%d L%d" % (A, L)
        assert (t[:, L:, :] == 0).all() and (t[:, :, L:] == 0).all(), "A%d L%d: pad rows / columns" % (A, L)


def _relpos(wd, A, L, Lr):
    o = dict(table=Buf(A, Lr, Lr))
    T.call("tnr_relpos_table", wd, A, L, o["table"].t)
    return o


# ------------------------------------------------------------------------------------------------ refusals
def test_argument_checks_refuse_before_any_launch():
    """Each bad call raises with the library's error code and the tnr_last_error text of THAT check, and no output is touched."""
    td, H, M, L, Q = torch.bfloat16, 256, 8, 4, 8
    out16, out32, out32b = Buf(4096, dtype=td), Buf(4096), Buf(4096)
    x16 = torch.zeros(8192, device=DEV, dtype=td)
    f32 = torch.zeros(8192, device=DEV)
    i64 = torch.zeros(8192, device=DEV, dtype=torch.int64)
    i32 = torch.zeros(8192, device=DEV, dtype=torch.int32)
    site = T.Dropout.site_of(0.1, 1, T.DROP_FFN_OUT, 0, 1)
    ln_f = lambda h: ("tnr_ln_fwd", x16, f32, f32, R.EPS, out16.t, out32.t, M, h)
    ln_b = lambda h, dg, part: ("tnr_ln_bwd", x16, x16, f32, f32, out16.t, dg, None, None, part, M, h)
    emb = lambda l, h: ("tnr_embed_ln_fwd", i64, 2, l, h, f32, f32, f32, f32, f32, R.EPS, out16.t, out32.t)
    embi = lambda l, h: ("tnr_embed_ln_fwd_indexed", i32, i32, 2, l, h, f32, f32, f32, f32, f32, R.EPS, out16.t, out32.t)
    ap_f = lambda l, lde: ("tnr_attpool_fwd", x16, f32, lde, f32, f32, Q, out32.t, out32b.t, out32b.t, 2, l, H)
    ap_b = lambda l, lde, ldd: ("tnr_attpool_bwd", x16, f32, lde, f32, Q, f32, f32, f32, out16.t, out16.t, ldd, out32.t, out32b.t, None, 2, l, H)
    ap_fl = lambda l, lde: ("tnr_attpool_fwd_long", x16, f32, lde, f32, f32, Q, out32.t, out32b.t, out32b.t, f32, 2, l, H)
    ap_bl = lambda l, lde, ldd: ("tnr_attpool_bwd_long", x16, f32, lde, f32, Q, f32, f32, out16.t, out16.t, ldd, out32.t, out32b.t, None, f32, 2, l, H)
    bad = [("ln_fwd H = 384", ln_f(384), "H must be"), ("ln_bwd H = 384", ln_b(384, None, None), "H must be"),
           ("embed H = 384", emb(L, 384), "H must be"), ("embed L = 0", emb(0, H), "1<=L<=512"), ("embed L = 513", emb(513, H), "1<=L<=512"),
           ("embed indexed H = 384", embi(L, 384), "H must be"), ("embed indexed L = 0", embi(0, H), "1<=L<=512"),
           ("embed indexed L = 513", embi(513, H), "1<=L<=512"),
           ("attpool_fwd L = 0", ap_f(0, Q), "bad shape"), ("attpool_fwd L = 513", ap_f(513, Q), "bad shape"),
           ("attpool_fwd lde < Q", ap_f(L, Q - 1), "bad shape"), ("attpool_bwd L = 513", ap_b(513, Q, Q), "bad shape"),
           ("attpool_bwd lde < Q", ap_b(L, Q - 1, Q), "bad shape"), ("attpool_bwd lddpre < Q", ap_b(L, Q, Q - 1), "bad shape"),
           ("attpool_fwd_long L = 513", ap_fl(513, Q), "bad shape"), ("attpool_fwd_long lde < Q", ap_fl(L, Q - 1), "bad shape"),
           ("attpool_bwd_long L = 0", ap_bl(0, Q, Q), "bad shape"), ("attpool_bwd_long lde < Q", ap_bl(L, Q - 1, Q), "bad shape"),
           ("attpool_bwd_long lddpre < Q", ap_bl(L, Q, Q - 1), "bad shape"),
           ("relpos L = 0", ("tnr_relpos_table", f32, 2, 0, out32.t), "1<=L<=512"),
           ("relpos L = 513", ("tnr_relpos_table", f32, 2, 513, out32.t), "1<=L<=512"),
           ("colsum ldx % 4", ("tnr_colsum", x16, 10, T.BF16, M, 8, out32.t, out32b.t, 0), "tnr_colsum: bad argument"),
           ("ln_bwd_do site without dxm", ("tnr_ln_bwd_do", x16, x16, f32, f32, out16.t, None, None, None, None, M, H, None, site),
            "masked second output"),
           ("ln_bwd dgamma without part", ln_b(H, out32.t, None), "part workspace")]
    for what, args, word in bad:
        with pytest.raises(T.TnrError) as ei:
            T.call(*args)
        msg = str(ei.value)
        assert "failed (" in msg and "failed (0)" not in msg and word in msg.split("): ", 1)[1], what + ": refused for another reason: " + msg
    torch.cuda.synchronize()
    for b in (out16, out32, out32b):
        assert (b.raw == SENT).all(), "a refused call wrote to an output"
