"""The fp32 head, loss and optimiser kernels (csrc/heads.hip, optim.hip, util_f32.hip), one by one, against the float64 references of
tests/heads_ref.py (tied to the oracle by tests/test_heads_ref_cpu.py), at the smallest shapes that reach each branch: tails and
second blocks of the fused user encoder, the rounds of the one-workgroup loss kernel, the short / unrolled / tail loops of the
segment sum and of the descriptor reduction, the scalar tail and the guarded bias corrections of the optimiser.

Every output buffer has a sentinel region behind it that must come back untouched, and every kernel runs twice and must give the
same bits (include/tnr_hip.h promises a fixed summation order).

Bounds.  |got - ref| <= rtol |ref| + floor max|ref|, ref in float64.
  * Pure fixed-order sums (segment sum, tnr_reduce_multi, the blend / score scatters): the derived bound count * 2^-23 * sum|terms|
    of tests/test_embed_train_kernels_gpu.py::test_scatter_sum_rows_against_float64_index_add; count = number of terms (+ 1 where
    each term is itself a rounded product, + 1 for a scale factor).
  * Everything behind __expf / __logf / tnr_tanh / a reciprocal keeps the ceiling tests/test_kernels_gpu.py holds that output to:
    forward outputs and losses 1e-4, dvec 1e-3, dscore 1e-3, NRMS ctx 2e-4 (floor 1e-5 of the tensor's largest magnitude: an
    element that cancels carries the absolute rounding error of terms no larger than that magnitude, 1e-5 is ~ 84 ulp of it, and it
    is below every absolute floor test_kernels_gpu.py uses on its O(1) data); parameter-gradient partials and NRMS dqkv 2e-3 with
    floor 2e-3 max|ref|; the optimiser rtol 1e-5, atol 1e-6.  dpre, the gradient of the fc1 pre-activation, feeds both dvec and
    dW1 and is held to the tighter of the two (1e-3).
  * The fc2 bias partial is a cancelling sum (zero in exact arithmetic, heads_ref.user_bwd): held absolutely against 2e-3 of the
    largest fc2 WEIGHT partial, its neighbour.  Nothing else is exempted.
Every comparison prints its largest error and that error as a fraction of its bound (EXPERIMENTS.md item 61 records them)."""
import struct

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import heads_ref as R                          # noqa: E402
import tnr_hip as T                            # noqa: E402

DEV = "cuda:0"
SENT = -7.25
GUARD = 64
FLOOR = 1e-5
FWD, DVEC, DSCORE, CTX, PART = 1e-4, 1e-3, 1e-3, 2e-4, 2e-3
U23 = 2.0 ** -23


def rnd(shape, seed, scale=1.0):
    return (np.random.RandomState(seed).standard_normal(shape) * scale).astype(np.float32)


def dev(x, dt=None):
    t = torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    return t.to(dt) if dt is not None else t


def host(t):
    return t.float().cpu().numpy().astype(np.float64)


class Buf:
    """An output buffer of `shape` with GUARD sentinel elements behind it."""

    def __init__(self, *shape, fill=SENT, dtype=torch.float32):
        n = int(np.prod(shape))
        self.raw = torch.full((n + GUARD,), SENT, device=DEV, dtype=dtype)
        self.t = self.raw[:n].view(*shape)
        if isinstance(fill, np.ndarray):
            self.t.copy_(dev(fill.astype(np.float32)).view(*shape))
        elif fill != SENT:
            self.t.fill_(fill)

    def guard_ok(self):
        return bool((self.raw[self.t.numel():] == SENT).all())


def twice(fn):
    """fn() -> {name: Buf}: run it twice, require untouched guards and equal bits, -> {name: float64 numpy}."""
    a = fn()
    b = fn()
    torch.cuda.synchronize()
    for n in a:
        assert a[n].guard_ok() and b[n].guard_ok(), "%s: wrote behind its buffer" % n
        assert torch.equal(a[n].t.view(torch.int32), b[n].t.view(torch.int32)), "%s: two runs differ" % n
    return {n: host(a[n].t) for n in a}


def check(what, got, want, rtol, floor=FLOOR):
    """|got - want| <= rtol |want| + floor max|want|, printing the largest error and the worst error / bound."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, what
    bound = rtol * np.abs(want) + floor * np.abs(want).max(initial=0.0)
    _report(what, got, want, bound)


def check_abs(what, got, want, rtol, atol):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, what
    _report(what, got, want, atol + rtol * np.abs(want))


def check_sum(what, got, want, mag, count):
    """A fixed-order fp32 sum of `count` terms against the float64 sum: count * 2^-23 * sum|terms|, element by element."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, what
    _report(what, got, want, np.asarray(count, np.float64) * U23 * np.asarray(mag, np.float64))


def _report(what, got, want, bound):
    err = np.abs(got - want)
    ratio = np.where(err == 0.0, 0.0, err / np.maximum(bound, 1e-300))
    worst = float(ratio.max(initial=0.0))
    print("[heads-kernels] %s: max|err| %.3e, worst err / bound %.3f" % (what, float(err.max(initial=0.0)), worst))
    assert np.isfinite(got).all(), what
    assert (err <= bound).all(), "%s: %d of %d elements over the bound, worst err / bound %.3f" % (what, int((err > bound).sum()), err.size, worst)


def masks(B, U, seed):
    """(B >= 4, U): all ones, all zeros, a single one, random."""
    rs = np.random.RandomState(seed)
    m = (rs.rand(B, U) > 0.4).astype(np.float32)
    m[0], m[1], m[2] = 1, 0, 0
    m[2, rs.randint(U)] = 1
    return m


def user_params(nm, D, Q, seed):
    return dict(pad=rnd((nm, D), seed), w1=rnd((nm, Q, D), seed + 1, 0.05), b1=rnd((nm, Q), seed + 2, 0.05),
                w2=rnd((nm, Q), seed + 3, 0.2), b2=rnd((nm,), seed + 4, 0.05))


# ------------------------------------------------------------------------------------------------ tnr_user_score_fwd
def _user_inputs(nm, B, U, C, D, Q, seed):
    rs = np.random.RandomState(seed)
    Rr = 2 * U + 9
    vec = rnd((nm, Rr, D), seed + 1, 0.3)
    hidx = rs.randint(0, Rr, (B, U)).astype(np.int32)
    if U > 1:
        hidx[0, 1] = hidx[0, 0]                      # a row twice inside one impression
        hidx[3] = hidx[2][::-1]                      # the same rows in two impressions (the forward only reads them)
    cidx = rs.randint(0, Rr, (B, C)).astype(np.int32)
    cidx[0, 0] = hidx[0, 0]                          # a candidate that is also a history row
    return Rr, vec, hidx, cidx, masks(B, U, seed + 2), user_params(nm, D, Q, seed + 3)


def _user_ref(vec, hidx, cidx, mask, pr, ulm):
    out = []
    for z in range(vec.shape[0]):
        hv = R.blend(vec[z], hidx, mask, pr["pad"][z], ulm)
        f = R.user_fwd(hv, mask, pr["w1"][z], pr["b1"][z], pr["w2"][z], pr["b2"][z], ulm)
        f["score"] = R.score_fwd(vec[z], cidx, f["user"])
        out.append(f)
    return {k: np.stack([f[k] for f in out], 0) for k in ("user", "score", "e", "alpha", "den")}


def _user_run(route, nm, B, U, C, D, Q, ulm, Rr, vec, hidx, cidx, mask, pr, epad_given=False):
    dv = {k: dev(v) for k, v in pr.items()}
    epre = epad = None
    if route == "epre":            # fc1 of every UNBLENDED history slot, and fc1(pad_doc) for the replaced ones
        pre = np.einsum("zrd,zqd->zrq", R.f64(vec)[:, hidx.reshape(-1)], R.f64(pr["w1"])) + R.f64(pr["b1"])[:, None, :]
        epre = dev(pre.astype(np.float32))
        if epad_given:
            epad = dev((np.einsum("zd,zqd->zq", R.f64(pr["pad"]), R.f64(pr["w1"])) + R.f64(pr["b1"])).astype(np.float32))
    stride = B * D + 8
    args = (dev(vec), Rr, dev(hidx), dev(cidx), dev(mask), dv["pad"], dv["w1"], dv["b1"], dv["w2"], dv["b2"], ulm, epre, epad)

    def fn():
        o = dict(user=Buf(nm, stride), score=Buf(nm, B, C), e=Buf(nm, B, U, Q), alpha=Buf(nm, B, U), den=Buf(nm, B))
        T.call("tnr_user_score_fwd", *args, o["user"].t, stride, o["score"].t, o["e"].t, o["alpha"].t, o["den"].t, nm, B, U, C, D, Q)
        return o
    got = twice(fn)
    assert (got["user"][:, B * D:] == SENT).all(), "user: wrote between the models' blocks"
    got["user"] = got["user"][:, :B * D].reshape(nm, B, D)
    return got


BASE = (33, 40, 36, 5)
USER_SHAPES = sorted({(U, BASE[1], BASE[2], BASE[3]) for U in (1, 31, 32, 33, 64)} |
                     {(BASE[0], D, BASE[2], BASE[3]) for D in (8, 24, 40, 64, 72, 256)} |
                     {(BASE[0], BASE[1], Q, BASE[3]) for Q in (4, 28, 32, 36, 200)} |
                     {(BASE[0], BASE[1], BASE[2], C) for C in (1, 5, 17)} | {(50, 256, 200, 5)})


def _user_both_routes(tag, nm, B, U, C, D, Q, ulm, seed, fused=True, epre=True, epad_given=False):
    inp = _user_inputs(nm, B, U, C, D, Q, seed)
    ref = _user_ref(inp[1], inp[2], inp[3], inp[4], inp[5], ulm)
    got = {}
    if fused:
        got["fused"] = _user_run("fused", nm, B, U, C, D, Q, ulm, *inp)
    if epre:
        got["epre"] = _user_run("epre", nm, B, U, C, D, Q, ulm, *inp, epad_given=epad_given)
    for route, g in got.items():
        for k in ("user", "score", "e", "alpha", "den"):
            check("user_score_fwd/%s/%s %s" % (route, k, tag), g[k], ref[k], FWD)
    if fused and epre:             # the two routes against each other, at the bound of tests/test_kernels_gpu.py::test_user_score_fwd_bwd
        for k in ("e", "alpha", "den"):
            check_abs("user_score_fwd/routes/%s %s" % (k, tag), got["fused"][k], got["epre"][k], 2e-5, 2e-6)
    if ulm:                        # an all-zero mask row: weights, user vector and scores exactly zero
        for g in got.values():
            assert (g["alpha"][:, 1] == 0).all() and (g["user"][:, 1] == 0).all() and (g["score"][:, 1] == 0).all()
    return got


@pytest.mark.parametrize("ulm", [0, 1])
@pytest.mark.parametrize("U,D,Q,C", USER_SHAPES)
def test_user_score_fwd_both_routes(U, D, Q, C, ulm):
    _user_both_routes("U%d D%d Q%d C%d ulm%d" % (U, D, Q, C, ulm), 2, 4, U, C, D, Q, ulm, 100 + U + D + Q + C,
                      epad_given=bool(Q % 8))


@pytest.mark.parametrize("ulm", [0, 1])
def test_user_score_fwd_one_model(ulm):
    U, D, Q, C = BASE
    _user_both_routes("one model ulm%d" % ulm, 1, 4, U, C, D, Q, ulm, 7, epad_given=True)


def test_user_score_fwd_D_4_mod_8_is_refused_on_the_fused_route_only():
    nm, B, U, C, D, Q = 2, 4, 33, 5, 44, 36
    inp = _user_inputs(nm, B, U, C, D, Q, 9)
    with pytest.raises(T.TnrError):
        _user_run("fused", nm, B, U, C, D, Q, 0, *inp)
    _user_both_routes("D44", nm, B, U, C, D, Q, 0, 9, fused=False)


def test_user_score_fwd_at_and_over_the_lds_cap():
    """64 (D + 4) + U Q + D + 64 floats (fused) and U D + U Q + D + Q + 68 floats (epre) against 160 KB: U = 64, Q = 200 fits up to
    D = 424 / 428 and is refused, before any launch, at D = 432."""
    nm, B, U, C, Q = 1, 4, 64, 5, 200
    _user_both_routes("lds fused D424", nm, B, U, C, 424, Q, 0, 21, epre=False)
    _user_both_routes("lds epre D428", nm, B, U, C, 428, Q, 1, 22, fused=False)
    inp = _user_inputs(nm, B, U, C, 432, Q, 23)
    for route in ("fused", "epre"):
        with pytest.raises(T.TnrError):
            _user_run(route, nm, B, U, C, 432, Q, 0, *inp)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ user encoder backward
@pytest.mark.parametrize("ulm", [0, 1])
@pytest.mark.parametrize("U,D,Q,repeat", [(1, 8, 4, False), (31, 24, 28, False), (33, 40, 36, True), (64, 72, 32, False),
                                          (50, 256, 200, True)])
def test_user_bwd_chain(U, D, Q, repeat, ulm):
    """tnr_user_bwd_pre -> dW1 = dpre^T hv, dhv = dpre W1 (tnr_sgemm) -> tnr_user_bwd_post: the chain the engine issues.  Rows are
    distinct across impressions; `repeat` names one row twice inside impression 0, whose gradient is then the sum of both slots."""
    B, seed = 4, 300 + U + ulm
    rs = np.random.RandomState(seed)
    Rr = B * U + 5
    vec = rnd((Rr, D), seed + 1, 0.3)
    hidx = rs.permutation(Rr)[:B * U].reshape(B, U).astype(np.int32)
    if repeat:
        hidx[0, U - 1] = hidx[0, 2]
    mask = masks(B, U, seed + 2)
    pr = user_params(1, D, Q, seed + 3)
    hv = R.blend(vec, hidx, mask, pr["pad"][0], ulm)
    f = R.user_fwd(hv, mask, pr["w1"][0], pr["b1"][0], pr["w2"][0], pr["b2"][0], ulm)
    e32, a32 = f["e"].astype(np.float32), f["alpha"].astype(np.float32)
    f = dict(e=R.f64(e32), alpha=R.f64(a32))                  # what the kernels are handed
    duser, base = rnd((B, D), seed + 4), rnd((Rr, D), seed + 5)
    b = R.user_bwd(hv, mask, pr["w1"][0], pr["w2"][0], f, duser, ulm)
    dvec_ref, _ = R.scatter(hidx, b["dslot"], Rr, base=base)
    ps = T.query("tnr_user_bwd_part_stride", D, Q)
    assert ps == 2 * Q + D + 1
    w1 = dev(pr["w1"][0])

    def fn():
        o = dict(hv=Buf(B * U, D), dpre=Buf(B * U, Q), part=Buf(B, ps), dvec=Buf(Rr, D, fill=base), dw1=Buf(Q, D), dhv=Buf(B * U, D))
        sg = torch.zeros(8 * Q * D, device=DEV)
        T.call("tnr_user_bwd_pre", dev(vec), dev(hidx), dev(mask), dev(pr["pad"][0]), dev(pr["w2"][0]), ulm, dev(duser), dev(e32),
               dev(a32), o["hv"].t, o["dpre"].t, o["part"].t, B, U, D, Q)
        T.call("tnr_sgemm", o["dpre"].t, 1, Q, 0, None, o["hv"].t, 1, D, 0, o["dw1"].t, D, 0, None, 0, Q, D, B * U, 1, 1.0, 0.0, 8, sg)
        T.call("tnr_sgemm", o["dpre"].t, Q, 1, 0, None, w1, 1, D, 0, o["dhv"].t, D, 0, None, 0, B * U, D, Q, 1, 1.0, 0.0, 1, None)
        T.call("tnr_user_bwd_post", o["dhv"].t, dev(a32), dev(duser), dev(mask), dev(hidx), ulm, o["dvec"].t, o["part"].t, B, U, D, Q)
        return o
    got = twice(fn)
    tag = "U%d D%d Q%d ulm%d" % (U, D, Q, ulm)
    m = R.f64(mask)[..., None]
    mag = np.abs(hv) if ulm else np.abs(R.f64(vec)[hidx] * m) + np.abs(R.f64(pr["pad"][0]) * (1 - m))
    check_sum("user_bwd/hv " + tag, got["hv"].reshape(B, U, D), hv, mag, 2)
    check("user_bwd/dpre " + tag, got["dpre"].reshape(B, U, Q), b["dpre"], DVEC)
    check("user_bwd/dvec " + tag, got["dvec"], dvec_ref, DVEC)
    check("user_bwd/dW1 " + tag, got["dw1"], b["dW1"], PART, PART)
    p = got["part"]
    check("user_bwd/part_b1 " + tag, p[:, :Q], b["part_b1"], PART, PART)
    check("user_bwd/part_w2 " + tag, p[:, Q:2 * Q], b["part_w2"], PART, PART)
    check("user_bwd/part_pad " + tag, p[:, 2 * Q:2 * Q + D], b["part_pad"], PART, PART)
    # the fc2 bias partial: a cancelling sum, held absolutely against its neighbour, the fc2 weight partial
    check_abs("user_bwd/part_b2 " + tag, p[:, 2 * Q + D], b["part_b2"], 0.0, PART * np.abs(b["part_w2"]).max())


# ------------------------------------------------------------------------------------------------ blend, scorer backward, gather
@pytest.mark.parametrize("ulm", [0, 1])
@pytest.mark.parametrize("D", [4, 36, 256])
def test_user_blend_fwd_bwd(D, ulm):
    nm, B, U, seed = 2, 4, 7, 40 + D
    rs = np.random.RandomState(seed)
    Rr = B * U + 3
    vec, pad = rnd((nm, Rr, D), seed, 0.5), rnd((nm, D), seed + 1)
    hidx = rs.permutation(Rr)[:B * U].reshape(B, U).astype(np.int32)
    hidx[0, U - 1] = hidx[0, 1]                       # within one impression: summed in slot order
    mask = masks(B, U, seed + 2)
    got = twice(lambda: _blend_fwd(vec, Rr, hidx, mask, pad, ulm, nm, B, U, D))
    for z in range(nm):
        hv = R.blend(vec[z], hidx, mask, pad[z], ulm)
        m = R.f64(mask)[..., None]
        mag = np.abs(hv) if ulm else np.abs(R.f64(vec[z])[hidx] * m) + np.abs(R.f64(pad[z]) * (1 - m))
        check_sum("blend_fwd/hv D%d ulm%d" % (D, ulm), got["hv"][z].reshape(B, U, D), hv, mag, 2)
    dhv, base, stride = rnd((B, U, D), seed + 3), rnd((Rr, D), seed + 4), D + 5

    def bwd():
        o = dict(dvec=Buf(Rr, D, fill=base), part=Buf(B, stride))
        T.call("tnr_user_blend_bwd", dev(dhv.reshape(B * U, D)), dev(mask), dev(hidx), ulm, o["dvec"].t, o["part"].t[:, 5:], stride, B, U, D)
        return o
    got = twice(bwd)
    m = np.ones((B, U, 1)) if ulm else R.f64(mask)[..., None]
    want, mag = R.scatter(hidx, R.f64(dhv) * m, Rr, base=base)
    check_sum("blend_bwd/dvec D%d ulm%d" % (D, ulm), got["dvec"], want, mag, 3)
    assert (got["part"][:, :5] == SENT).all()
    check_sum("blend_bwd/pad_part D%d ulm%d" % (D, ulm), got["part"][:, 5:], (R.f64(dhv) * (1 - m)).sum(1), np.abs(R.f64(dhv) * (1 - m)).sum(1), U)


def _blend_fwd(vec, Rr, hidx, mask, pad, ulm, nm, B, U, D):
    o = dict(hv=Buf(nm, B * U, D))
    T.call("tnr_user_blend_fwd", dev(vec), Rr, dev(hidx), dev(mask), dev(pad), ulm, o["hv"].t, nm, B, U, D)
    return o


@pytest.mark.parametrize("C", [1, 5, 17])
@pytest.mark.parametrize("D", [4, 100, 300])
def test_score_bwd(D, C):
    B, seed = 4, 60 + D + C
    rs = np.random.RandomState(seed)
    Rr = B * C + 3
    vec, user, dscore = rnd((Rr, D), seed), rnd((B, D), seed + 1), rnd((B, C), seed + 2)
    cidx = rs.permutation(Rr)[:B * C].reshape(B, C).astype(np.int32)
    if C > 1:
        cidx[0, C - 1] = cidx[0, 0]
    base, ubase = rnd((Rr, D), seed + 3), rnd((B, D), seed + 4)

    def fn():
        o = dict(dvec=Buf(Rr, D, fill=base), duser=Buf(B, D, fill=ubase))
        T.call("tnr_score_bwd", dev(vec), dev(cidx), dev(user), dev(dscore), o["dvec"].t, o["duser"].t, B, C, D)
        return o
    got = twice(fn)
    dcand, duser = R.score_bwd(vec, cidx, user, dscore)
    want, mag = R.scatter(cidx, dcand, Rr, base=base)
    check_sum("score_bwd/dvec D%d C%d" % (D, C), got["dvec"], want, mag, 4)       # base + two slots at most, each a rounded product
    umag = np.abs(R.f64(ubase)) + np.einsum("bc,bcd->bd", np.abs(R.f64(dscore)), np.abs(R.f64(vec)[cidx]))
    check_sum("score_bwd/duser D%d C%d" % (D, C), got["duser"], R.f64(ubase) + duser, umag, C + 2)


def test_gather_rows_with_a_row_offset():
    nm, Rr, D, n, rows, row0 = 2, 30, 4, 21, 29, 6
    tbl = rnd((nm, Rr, D), 1)
    idx = np.random.RandomState(2).randint(0, Rr, n).astype(np.int32)
    got = twice(lambda: _gather(tbl, Rr, idx, n, D, nm, rows, row0))["out"]
    assert np.array_equal(got[:, row0:row0 + n], R.f64(tbl)[:, idx])
    assert (got[:, :row0] == SENT).all() and (got[:, row0 + n:] == SENT).all()


def _gather(tbl, Rr, idx, n, D, nm, rows, row0):
    o = dict(out=Buf(nm, rows, D))
    T.call("tnr_gather_rows", dev(tbl), Rr, dev(idx), n, D, nm, o["out"].t, rows, row0)
    return o


# ------------------------------------------------------------------------------------------------ NRMS self-attention
@pytest.mark.parametrize("use_mask", [0, 1])
@pytest.mark.parametrize("NH,U,nm", [(1, 1, 1), (3, 17, 2), (16, 50, 2), (16, 64, 1), (3, 64, 2), (1, 50, 1)])
def test_nrms_attn_fwd_bwd(NH, U, nm, use_mask):
    B, Dh, seed = 4, NH * 16, 500 + NH + U
    hv = rnd((nm, B * U, Dh), seed, 0.5)
    W, bq = rnd((nm, 3 * Dh, Dh), seed + 1, 2.0 / np.sqrt(Dh)), rnd((nm, 3 * Dh), seed + 2, 0.1)
    qkv = (np.einsum("zrd,zjd->zrj", R.f64(hv), R.f64(W)) + R.f64(bq)[:, None, :]).astype(np.float32)
    mask = masks(B, U, seed + 3)
    ref = [R.nrms_fwd(qkv[z].reshape(B, U, 3 * Dh), mask, use_mask, NH) for z in range(nm)]
    assert max(f["arg_max"] for f in ref) < 30.0            # the raw exp stays finite in fp32 by construction
    rows = B * U + 3

    def fwd():
        o = dict(ctx=Buf(nm, rows, Dh))
        T.call("tnr_nrms_attn_fwd", dev(qkv), dev(mask), use_mask, o["ctx"].t, rows, nm, B, U, NH)
        return o
    ctx = twice(fwd)["ctx"]
    tag = "NH%d U%d mask%d" % (NH, U, use_mask)
    assert (ctx[:, B * U:] == SENT).all()
    for z in range(nm):
        check("nrms_fwd/ctx " + tag, ctx[z, :B * U].reshape(B, U, Dh), ref[z]["ctx"], CTX)
    dctx = rnd((B, U, Dh), seed + 4)

    def bwd():
        o = dict(dqkv=Buf(B * U, 3 * Dh))
        T.call("tnr_nrms_attn_bwd", dev(qkv[0]), dev(mask), use_mask, dev(dctx.reshape(B * U, Dh)), o["dqkv"].t, B, U, NH)
        return o
    dqkv = twice(bwd)["dqkv"].reshape(B, U, 3 * Dh)
    check("nrms_bwd/dqkv " + tag, dqkv, R.nrms_bwd(ref[0], dctx), PART, PART)
    if use_mask:             # no key left: exactly zero context, finite and zero gradients
        assert (ctx[:, U:2 * U] == 0).all() and (dqkv[1] == 0).all()


# ------------------------------------------------------------------------------------------------ losses
@pytest.mark.parametrize("B,C,T_,tau,scale", [(1, 5, 4, 1.0, 1.0), (255, 2, 1, 0.5, 1.0), (256, 16, 16, 2.0, 1.0), (257, 1, 4, 1.0, 1.0),
                                              (600, 5, 0, 1.0, 1.0), (600, 16, 4, 0.5, 1.0), (37, 5, 16, 2.0, 1.0), (257, 16, 0, 2.0, 1.0),
                                              (300, 5, 4, 2.0, 30.0), (300, 2, 1, 0.5, 30.0)])
def test_kd_score_loss(B, C, T_, tau, scale):
    """scale 30: logits of magnitude 30 at temperature 0.5 / 2, where a missing max subtraction overflows or loses the small terms."""
    coef, seed = 0.2, B + C + T_
    s, ts = rnd((B, C), seed, scale), rnd((max(T_, 1), B, C), seed + 1, scale)
    y = np.random.RandomState(seed).randint(0, C, B)
    ref = R.kd_score_loss(s, ts if T_ else None, y, tau, coef)

    def fn():
        o = dict(tw=Buf(B, max(T_, 1)), dscore=Buf(B, C), losses=Buf(4))
        T.call("tnr_kd_score_loss", dev(s), dev(ts) if T_ else None, dev(y), tau, coef, o["tw"].t if T_ else None, o["dscore"].t,
               o["losses"].t, B, C, T_)
        return o
    got = twice(fn)
    tag = "B%d C%d T%d tau%g x%g" % (B, C, T_, tau, scale)
    if T_:
        check("kd_score/tw " + tag, got["tw"], ref["tw"], FWD)
    else:
        assert (got["tw"] == SENT).all()
    check("kd_score/distill " + tag, got["losses"][0], ref["distill"], FWD, 0.0)
    check("kd_score/target " + tag, got["losses"][1], ref["target"], FWD, 0.0)
    assert (got["losses"][2:] == SENT).all()
    check("kd_score/dscore " + tag, got["dscore"], ref["dscore"], DSCORE)


def test_kd_score_loss_refuses_more_than_16_candidates_or_teachers():
    B = 8
    tw, dscore, losses = Buf(B, 17), Buf(B, 17), Buf(4)
    for C, T_ in ((17, 4), (5, 17)):
        with pytest.raises(T.TnrError):
            T.call("tnr_kd_score_loss", dev(rnd((B, C), 1)), dev(rnd((T_, B, C), 2)), dev(np.zeros(B, np.int64)), 1.0, 0.2, tw.t,
                   dscore.t, losses.t, B, C, T_)
    torch.cuda.synchronize()
    assert (tw.raw == SENT).all() and (dscore.raw == SENT).all() and (losses.raw == SENT).all()


@pytest.mark.parametrize("B,U,C,D,T_", [(3, 0, 4, 4, 1), (3, 6, 2, 260, 4), (3, 0, 2, 768, 4), (5, 50, 4, 64, 1), (4, 2, 1, 768, 1)])
def test_kd_embed_loss(B, U, C, D, T_):
    rt = B * (U + C + 1)                       # 15, 27, 9, 275 rows: a last block of four that is not full; 16: one that is
    S, P = rnd((rt, D), D, 0.3), rnd((T_, rt, D), D + 1, 0.3)
    tw = np.exp(R.log_softmax(rnd((B, T_), D + 2))).astype(np.float32)
    loss, dS, dP = R.kd_embed_loss(S, P, tw, B, U, C)

    def fn():
        o = dict(loss=Buf(1), dS=Buf(rt, D), dP=Buf(T_, rt, D), part=Buf(rt))
        T.call("tnr_kd_embed_loss", dev(S), dev(P), dev(tw), o["loss"].t, o["dS"].t, o["dP"].t, o["part"].t, B, U, C, D, T_)
        return o
    got = twice(fn)
    tag = "B%d U%d C%d D%d T%d" % (B, U, C, D, T_)
    check("kd_embed/loss " + tag, got["loss"][0], loss, FWD, 0.0)
    check("kd_embed/dS " + tag, got["dS"], dS, FWD)
    check("kd_embed/dP " + tag, got["dP"], dP, FWD)


# ------------------------------------------------------------------------------------------------ fixed-order sums
SEG_LENS = [0, 1, 4, 5, 16, 17, 63, 64, 65, 113, 300, 0]


@pytest.mark.parametrize("D", [4, 64, 252, 256, 260, 768, 2048])
def test_segment_sum_rows(D):
    """Segment lengths on both sides of the <= 4 shortcut, of the 64-wide unrolled loop and of its 16-wide tail; empty first and
    last segments; `order` a scattered permutation into a taller src."""
    rs = np.random.RandomState(D)
    n, tall = sum(SEG_LENS), sum(SEG_LENS) + 57
    src = rnd((tall, D), D + 1)
    order = rs.permutation(tall)[:n].astype(np.int32)
    seg = np.concatenate([[0], np.cumsum(SEG_LENS)]).astype(np.int32)
    want, mag = R.segment_sum(src, order, seg)

    def fn():
        o = dict(out=Buf(len(SEG_LENS), D))
        T.call("tnr_segment_sum_rows", dev(src), dev(order), dev(seg), len(SEG_LENS), D, o["out"].t)
        return o
    got = twice(fn)["out"]
    assert (got[0] == 0).all() and (got[-1] == 0).all()
    check_sum("segment_sum D%d" % D, got, want, mag, np.asarray(SEG_LENS, np.float64)[:, None])


@pytest.mark.parametrize("D", [6, 2052])
def test_segment_sum_rows_refuses_bad_widths(D):
    out = Buf(2, D)
    with pytest.raises(T.TnrError):
        T.call("tnr_segment_sum_rows", dev(rnd((4, D), 1)), dev(np.arange(4, dtype=np.int32)), dev(np.array([0, 2, 4], np.int32)), 2, D, out.t)
    torch.cuda.synchronize()
    assert (out.raw == SENT).all()


RED_ROWS, RED_COLS, RED_SCALES = [1, 2, 3, 4, 5, 7, 8, 9, 12, 13, 100], [1, 63, 64], [1.0, 0.5, 1.0 / 1024]


def _reduce_jobs():
    """(rows, ncols, stride, accumulate, scale, source offset, destination offset) for every rows x ncols; destinations 3 floats
    apart so that every neighbour is a sentinel."""
    jobs, so, do = [], 0, 3
    for i, rows in enumerate(RED_ROWS):
        for j, nc in enumerate(RED_COLS):
            k = i * len(RED_COLS) + j
            stride = nc + 1 + (k % 5)
            jobs.append((rows, nc, stride, k % 2, RED_SCALES[(k // 2) % 3], so, do))
            so += rows * stride + 2
            do += nc + 3
    return jobs, so, do


@pytest.mark.parametrize("how", ["one table", "engine"])
def test_reduce_multi(how):
    """`one table`: every descriptor in a single launch (one workgroup walks all rows: both chains of the unrolled loop and its
    remainder).  `engine`: the same jobs through engine._ReduceBatch, which sums tall partials per row chunk in place first."""
    import engine as E
    jobs, n_src, n_dst = _reduce_jobs()
    src = rnd((n_src,), 77)
    dst0 = rnd((n_dst,), 78)
    is_dst = np.zeros(n_dst, bool)
    for rows, nc, stride, acc, scale, so, do in jobs:
        is_dst[do:do + nc] = True
    init = np.where(is_dst, dst0, np.float32(SENT))

    def fn():
        o = dict(dst=Buf(n_dst, fill=init))
        s = dev(src)
        if how == "engine":
            rb = E._ReduceBatch(DEV)
            for rows, nc, stride, acc, scale, so, do in jobs:
                rb.add(s[so:], rows, stride, nc, o["dst"].t[do:], acc, scale)
            rb.flush()
        else:
            bits = lambda x: 0 if x == 1.0 else struct.unpack("<I", struct.pack("<f", x))[0]
            tab = [(s.data_ptr() + 4 * so, rows, stride, nc, o["dst"].t.data_ptr() + 4 * do, acc | (bits(scale) << 32))
                   for rows, nc, stride, acc, scale, so, do in jobs]
            T.call("tnr_reduce_multi", torch.tensor(tab, dtype=torch.int64, device=DEV), len(tab))
        torch.cuda.synchronize()               # s and the table stay alive until the launches are done
        return o
    got = twice(fn)["dst"]
    assert (got[~is_dst] == SENT).all(), "a neighbour of a destination was written"
    for rows, nc, stride, acc, scale, so, do in jobs:
        want, mag = R.reduce_desc(src[so:], rows, stride, nc, dst0[do:do + nc] if acc else None, scale)
        check_sum("reduce_multi/%s rows%d" % (how, rows), got[do:do + nc], want, mag, rows + 2)


# ------------------------------------------------------------------------------------------------ optimiser
HYPER = (1e-2, 0.9, 0.999, 1e-8)


def _opt_state(n, seed, ams):
    return [Buf(n, fill=rnd((n,), seed)), Buf(n, fill=0.0), Buf(n, fill=0.0), Buf(n, fill=0.0) if ams else None]


def _ptr(b):
    return b.t if b is not None else None


@pytest.mark.parametrize("ams", [1, 0])
@pytest.mark.parametrize("gs", [1.0, 0.125])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 1025, 4099])
def test_amsgrad_step_five_steps(n, gs, ams):
    grads = [rnd((n,), 900 + s) for s in range(5)]

    def fn():
        st = _opt_state(n, n, ams)
        trace = []
        for s in range(5):
            T.call("tnr_amsgrad_step", st[0].t, dev(grads[s]), st[1].t, st[2].t, _ptr(st[3]), n, s + 1, *HYPER, gs)
            trace.append([host(b.t) for b in st if b is not None])
        return dict(zip("pmvx", [b for b in st if b is not None])), trace
    (a, ta), (b, tb) = fn(), fn()
    torch.cuda.synchronize()
    for k in a:
        assert a[k].guard_ok() and b[k].guard_ok() and torch.equal(a[k].t, b[k].t)
    ref = [R.f64(rnd((n,), n)), np.zeros(n), np.zeros(n), np.zeros(n) if ams else None]
    for s in range(5):
        ref = list(R.adam_step(ref[0], grads[s], ref[1], ref[2], ref[3], s + 1, *HYPER, grad_scale=gs))
        for name, got, want in zip("pmvx", ta[s], [r for r in ref if r is not None]):
            check_abs("amsgrad/%s n%d gs%g ams%d step%d" % (name, n, gs, ams, s + 1), got, want, 1e-5, 1e-6)


def _guarded(n, ams, step, guard, stamp, known, gs=0.125):
    st = _opt_state(n, 5, ams)
    for b, sd in zip(st[1:], (6, 7, 8)):                        # a state in mid-training: m, v > 0, vmax >= v
        if b is not None:
            b.t.copy_(dev(np.abs(rnd((n,), sd, 0.1)) + (0.05 if sd == 8 else 0.0)))
    g = None if guard is None else torch.tensor(list(guard) + [0, 0], dtype=torch.int32, device=DEV)
    name = "tnr_amsgrad_step" if guard is None else "tnr_amsgrad_step_guarded"
    extra = () if guard is None else (g, stamp, known)
    T.call(name, st[0].t, dev(rnd((n,), 9)), st[1].t, st[2].t, _ptr(st[3]), n, step, *HYPER, gs, *extra)
    torch.cuda.synchronize()
    assert all(b.guard_ok() for b in st if b is not None)
    return [b.t.clone() for b in st if b is not None]


@pytest.mark.parametrize("ams", [1, 0])
@pytest.mark.parametrize("n", [5, 1025])
def test_amsgrad_step_guarded(n, ams):
    # (a) a launch whose stamp is the overflowed step's leaves everything as it was
    before = [b.t.clone() for b in _opt_state(n, 5, ams) if b is not None]
    st = _opt_state(n, 5, ams)
    g = torch.tensor([9, 1, 0, 0], dtype=torch.int32, device=DEV)
    T.call("tnr_amsgrad_step_guarded", st[0].t, dev(rnd((n,), 9)), st[1].t, st[2].t, _ptr(st[3]), n, 5, *HYPER, 1.0, g, 9, 0)
    torch.cuda.synchronize()
    assert all(torch.equal(x, b.t) for x, b in zip(before, [b for b in st if b is not None]))
    # (b) bias corrections of step - min(k, 2), k = guard[1] - known_skips; (c) never below step 1
    for step, skipped, known in ((5, 3, 3), (5, 4, 3), (5, 5, 3), (5, 6, 3), (5, 2, 0), (2, 1, 0), (2, 2, 0), (2, 3, 0), (1, 1, 0), (1, 2, 0)):
        k = skipped - known
        want = _guarded(n, ams, max(step - min(k, 2), 1), None, 0, 0)
        got = _guarded(n, ams, step, (3, skipped), 7, known)
        assert all(torch.equal(x, y) for x, y in zip(got, want)), "step %d, %d skips of which %d known" % (step, skipped, known)
    # ... and the corrections of different steps do differ, so the equalities above say something
    assert not torch.equal(_guarded(n, ams, 5, None, 0, 0)[0], _guarded(n, ams, 4, None, 0, 0)[0])
    assert not torch.equal(_guarded(n, ams, 4, None, 0, 0)[0], _guarded(n, ams, 3, None, 0, 0)[0])


# ------------------------------------------------------------------------------------------------ small utilities
@pytest.mark.parametrize("na,nb", [(0, 5), (5, 0), (255, 2), (256, 256), (300, 1), (1, 700)])
def test_concat_i32(na, nb):
    a, b = np.arange(1, na + 1, dtype=np.int32), -np.arange(1, nb + 1, dtype=np.int32)
    out = torch.full((na + nb + GUARD,), -7, dtype=torch.int32, device=DEV)
    T.call("tnr_concat_i32", dev(a) if na else None, na, dev(b) if nb else None, nb, out)
    torch.cuda.synchronize()
    assert np.array_equal(out[:na + nb].cpu().numpy(), np.concatenate([a, b])) and bool((out[na + nb:] == -7).all())


@pytest.mark.parametrize("n", [1, 255, 257])
def test_scale_inplace(n):
    x = rnd((n,), n)
    b = Buf(n, fill=x)
    T.call("tnr_scale_inplace", b.t, n, 0.3)
    torch.cuda.synchronize()
    assert np.array_equal(b.t.cpu().numpy(), x * np.float32(0.3)) and b.guard_ok()


def _cast_vector(n):
    """Ties of both 16-bit formats (to even, down and up), just beside them, fp32 and 16-bit denormals, values that round to
    infinity, signed zeros and infinities and a NaN, then random values."""
    bits = [0x3F808000, 0x3F818000, 0x3F808001, 0x3F807FFF, 0x3F801000, 0x3F803000, 0x3F801001, 0x3F800FFF,
            0x00000001, 0x00400000, 0x007FFFFF, 0x80000001, 0x807FFFFF, 0x7F7FFFFF, 0xFF7FFFFF, 0x477FE000, 0x477FF000, 0x477FEFFF,
            0x33800000, 0x33000000, 0x33000001, 0x38800000, 0x387FC000, 0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000]
    v = np.array(bits, np.uint32).view(np.float32)
    if n == 1:
        return v[:1]
    if n == 3:
        return v[[1, 9, 27]]                    # a tie, a denormal, the NaN
    return np.concatenate([v, rnd((n - len(v),), n, 3.0)])


@pytest.mark.parametrize("sfx,td", [("", torch.bfloat16), ("_f16", torch.float16)])
@pytest.mark.parametrize("n", [1, 3, 1025])
def test_casts_round_to_nearest_even(n, sfx, td):
    x = _cast_vector(n)
    want = torch.from_numpy(x).to(td)
    out = torch.full((n + GUARD,), 1.0, device=DEV, dtype=td)
    T.call("tnr_cast_f32_to_bf16" + sfx, dev(x), out, n)
    torch.cuda.synchronize()
    got = out[:n].cpu()
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan) and torch.equal(got.view(torch.int16)[~nan], want.view(torch.int16)[~nan])
    assert bool((out[n:] == 1.0).all())
    back = Buf(n)
    T.call("tnr_cast_bf16_to_f32" + sfx, dev(want.view(torch.int16).numpy()), back.t, n)
    torch.cuda.synchronize()
    g, w = back.t.cpu(), want.float()
    assert torch.equal(torch.isnan(g), nan) and torch.equal(g.view(torch.int32)[~nan], w.view(torch.int32)[~nan]) and back.guard_ok()
