"""The attention kernels (csrc/attn.hip: tnr_attn_l32_fwd / _bwd, tnr_attn_long_fwd / _bwd), one by one and in both builds, against
the float64 reference of tests/attn_ref.py on its case table: every L on both sides of the 4-row accumulator groups, the 8-row
staging passes, the 16-key MFMA halves and the 32-key tiles, pair counts that leave 1, 2 and 3 spare waves in a workgroup, long
workgroups with one live wave (L = 129 .. 160), odd tile counts through the double buffer, and masks that make the online softmax
rescale from -10000 to 0, at every tile or never (tests/test_attn_ref_cpu.py shows that the bounds are satisfiable and that each
seeded defect of the rounding model fails one of the checks made here).

Bounds (attn_ref's docstring derives them from the kernels' rounding points; u = 2^-8 bf16 / 2^-11 fp16, tiny = half the subnormal
spacing, U23 = 2^-23, no flat floor, every element compared):
  lse    min(1e-4 |lse|, 1e-4 (1 + |log l|) + U23 |lse|) + sum_k p_k e_s_k, e_s the fp32 score error, 2 U23 |mask| at a padded key;
  ctx    u |ctx| + tiny + sum_j ((u + rp_f) p_ij + tiny) |v_j| + fp32 sums, rp_f = e_s + sum_k p_k e_s_k + 2e-4 the relative error of a
         forward probability (rp = e_s + d lse + 1e-4 behind the stored lse in backward);
  delta  (long) what the stored 16-bit ctx carries, sum_d |dO| b_ctx, + the fp32 sum;
  dq/dk  u |.| + tiny + sum b_dS |k or q| / 8, b_dS = (u + rp) |dS| + tiny + p (d dP + d delta);   dv  the same over b_P and dO.
On top of the elementwise bounds, per output and case, ||kernel - ref||_F <= 2 ||model - ref||_F with attn_ref.emulate on the same
inputs: the worst-case sums above are 3 - 5 x wider than what a correct kernel does on the backward outputs, the model is not.

Every output is a Buf with a 64-element sentinel tail that must come back untouched; qkv, dctx and ctx-as-input have 8 rows of NaN
directly behind row N L (row indices are clamped to L - 1: nothing may read there); every call runs twice and must give equal bits;
rows L .. Lr of delta are exact zeros and of lse finite; the one-hot read-back holds every probability and every dS element of
every (sequence, head, query, key) to its own bound; each row of the l32 bias partials is held against the float64 column sum of
the kernel's own dqkv rows of that sequence; calls on a sub-range of the sequences and on the reversed batch give the same bits.
Every comparison prints its largest error, its worst err / bound and the Frobenius ratio (EXPERIMENTS.md item 66 records them)."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import attn_ref as AR                          # noqa: E402
import rows_ref as RR                          # noqa: E402
import tnr_hip as T                            # noqa: E402

DEV = "cuda:0"
SENT = AR.SENT                                 # exact in fp32, bf16 and fp16
GUARD = 64
NAN_ROWS = 8
NAN = float("nan")
D = AR.D


def dev32(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(DEV)


def dev_rows(x, dt):
    """x (M, C) on the device as dt with NAN_ROWS rows of NaN directly behind it (numpy or a device tensor of dt)."""
    t = torch.full((x.shape[0] + NAN_ROWS, x.shape[1]), NAN, device=DEV, dtype=dt)
    t[:x.shape[0]] = x if isinstance(x, torch.Tensor) else dev32(x).to(dt)
    return t


def host(t):
    return t.float().cpu().numpy().astype(np.float64)


class Buf:
    """An output buffer of `shape` filled with SENT, with GUARD sentinel elements behind it."""

    def __init__(self, *shape, dtype=torch.float32):
        n = int(np.prod(shape))
        self.raw = torch.full((n + GUARD,), SENT, device=DEV, dtype=dtype)
        self.t = self.raw[:n].view(*shape)

    def guard_ok(self):
        return bool((self.raw[self.t.numel():] == SENT).all())

    def bits(self):
        return self.t.view(torch.int16 if self.t.element_size() == 2 else torch.int32)

    def ptr(self, elems):
        return self.t.data_ptr() + elems * self.t.element_size()


def off(t, elems):
    return t.data_ptr() + elems * t.element_size()


@functools.lru_cache(maxsize=None)
def _ref(c, kind):
    """The float64 reference, its bounds and the rounding model of a table case: computed once, shared, never modified."""
    inp = AR.inputs(c, kind)
    r = AR.reference(inp)
    return inp, r, AR.bounds(r, kind, c.form), AR.emulate(kind, c.form, inp)


def device_inputs(inp, kind):
    td = RR.tdtype(kind)
    return dict(qkv=dev_rows(inp["qkv"], td), dctx=dev_rows(inp["dctx"], td), mask_add=dev32(inp["mask_add"]), rel=dev32(inp["rel"]))


def launch(form, kind, d, N, L, A, n0=0, bias=True):
    """Forward + backward on sequences n0 .. N - 1 through pointers offset into the full buffers -> {name: Buf} of full size (rows of
    the sequences in front of n0 keep their sentinel).  The long backward reads the forward's own ctx (copied in front of NaN
    rows), lse and delta buffers."""
    td, sfx = RR.tdtype(kind), RR.SFX[kind]
    Lp, HD, n = AR.pitch(form, L), A * D, N - n0
    o = dict(ctx=Buf(N * L, HD, dtype=td), dqkv=Buf(N * L, 3 * HD, dtype=td))
    qkv, dctx, madd = off(d["qkv"], n0 * L * 3 * HD), off(d["dctx"], n0 * L * HD), off(d["mask_add"], n0 * Lp)
    ctx, dqkv = o["ctx"].ptr(n0 * L * HD), o["dqkv"].ptr(n0 * L * 3 * HD)
    if form == "l32":
        o["bias_part"] = Buf(N, 3 * HD)
        T.call("tnr_attn_l32_fwd" + sfx, qkv, madd, d["rel"], ctx, n, L, A)
        T.call("tnr_attn_l32_bwd" + sfx, qkv, madd, d["rel"], dctx, dqkv, o["bias_part"].ptr(n0 * 3 * HD) if bias else None, n, L, A)
    else:
        o.update(lse=Buf(N, A, Lp), delta=Buf(N, A, Lp))
        lse, delta = o["lse"].ptr(n0 * A * Lp), o["delta"].ptr(n0 * A * Lp)
        T.call("tnr_attn_long_fwd" + sfx, qkv, madd, d["rel"], ctx, lse, n, L, A)
        ctx_in = dev_rows(o["ctx"].t, td)
        T.call("tnr_attn_long_bwd" + sfx, qkv, madd, d["rel"], off(ctx_in, n0 * L * HD), dctx, lse, delta, dqkv, n, L, A)
    return o


def twice(fn):
    """fn() -> {name: Buf}: run it twice, require equal bits -> ({name: float64 numpy, guard: {name: untouched}}, {name: Buf})."""
    a = fn()
    b = fn()
    torch.cuda.synchronize()
    for n in a:
        assert torch.equal(a[n].bits(), b[n].bits()), "%s: two runs differ" % n
    got = {n: host(a[n].t) for n in a}
    got["guard"] = {n: a[n].guard_ok() and b[n].guard_ok() for n in a}
    return got, a


# ------------------------------------------------------------------------------------------------ full operands
@pytest.mark.parametrize("kind", RR.KINDS)
@pytest.mark.parametrize("c", AR.CASES, ids=AR.case_id)
def test_attention_against_float64(c, kind):
    """ctx, lse, delta, dq, dk, dv element by element within their bounds and, per output, within twice the rounding model's
    Frobenius error; sentinels, NaN rows, equal bits, the padding rows of the statistics, (l32) each bias-partial row on its own and
    bias_part = NULL; the long backward runs on the forward's own lse and delta and must leave everything finite (all-pad, left-pad)."""
    form, N, L, A, _ = c
    inp, r, b, emu = _ref(c, kind)
    d = device_inputs(inp, kind)
    got, bufs = twice(lambda: launch(form, kind, d, N, L, A))
    bad, _ = AR.failures(kind, inp, r, b, got, emu, tag=AR.case_id(c))
    assert not bad, (AR.case_id(c), kind, bad)
    if form == "l32":
        got0, bufs0 = twice(lambda: launch(form, kind, d, N, L, A, bias=False))
        assert torch.equal(bufs["dqkv"].bits(), bufs0["dqkv"].bits()) and (got0["bias_part"] == SENT).all(), "bias_part = NULL"
        assert all(got0["guard"].values())


# ------------------------------------------------------------------------------------------------ one-hot read-back
def _onehot(N, L, A, w):
    """(N L, A 64): row r of every sequence holds e_(r - 64 w) in every head's 64 columns for r in window w, zeros elsewhere."""
    x = np.zeros((N, L, A, D))
    for r in range(64 * w, min(L, 64 * w + 64)):
        x[:, r, :, r - 64 * w] = 1.0
    return x.reshape(N * L, A * D)


ONEHOT = [AR.Case("l32", 3, 31, 3, "pad30"), AR.Case("l32", 5, 17, 1, "plain"), AR.Case("l32", 1, 32, 2, "sharp"),
          AR.Case("long", 2, 33, 1, "pad30"), AR.Case("long", 1, 97, 2, "sharp"), AR.Case("long", 1, 129, 2, "leftpad"),
          AR.Case("long", 1, 160, 1, "rising")]


@pytest.mark.parametrize("kind", RR.KINDS)
@pytest.mark.parametrize("c", ONEHOT, ids=AR.case_id)
def test_attention_one_hot_read_back(c, kind):
    """The head size is 64, so a one-hot operand over a 64-wide window turns an output into a copy of one slab of an inner matrix:
    V one-hot -> ctx = P[:, window], dctx one-hot -> dv = P^T, K one-hot -> dq = dS / 8, Q one-hot -> dk = dS^T / 8.  The general
    bounds on these inputs ARE the bounds of those elements (the sums have one term): every probability relative to itself, every
    dS element to its own size - every (sequence, head, query, key), both sides of every tile edge and of L.  Columns past the
    window are exact zeros."""
    form, N, L, A, _ = c
    HD = A * D
    base = AR.inputs(c, kind)
    for w in range((L + 63) // 64):
        width = min(L, 64 * w + 64) - 64 * w
        hot = _onehot(N, L, A, w)
        q, k, v = [base["qkv"][:, i * HD:(i + 1) * HD] for i in range(3)]
        for what, qkv, dctx, outs in (("V, dctx one-hot", (q, k, hot), hot, ("ctx", "dv")), ("K one-hot", (q, hot, v), base["dctx"], ("dq",)),
                                      ("Q one-hot", (hot, k, v), base["dctx"], ("dk",))):
            inp = dict(base, qkv=np.concatenate(qkv, 1), dctx=dctx)
            r = AR.reference(inp)
            b = AR.bounds(r, kind, form)
            d = device_inputs(inp, kind)
            got, _ = twice(lambda: launch(form, kind, d, N, L, A))
            tag = "%s w=%d %s" % (AR.case_id(c), w, what)
            bad, _ = AR.failures(kind, inp, r, b, got, None, tag=tag)
            assert not bad, (tag, kind, bad)
            g = AR.split(got, inp)
            for n in outs:
                assert (g[n][..., width:] == 0).all(), (tag, n, "columns past the window")
                assert (r[n][..., width:] == 0).all()


# ------------------------------------------------------------------------------------------------ sub-ranges, neighbours
@pytest.mark.parametrize("kind", RR.KINDS)
@pytest.mark.parametrize("c", [AR.Case("l32", 5, 9, 1, "plain"), AR.Case("long", 2, 129, 2, "lastdom")], ids=AR.case_id)
def test_attention_sub_range_and_reversed_batch(c, kind):
    """Engine calls these kernels on pointers offset into a joint buffer: sequences n0 .. N - 1 alone give the bits of their rows in
    the full call (with 5 pairs every n0 moves each pair to another wave of its workgroup) and leave the rows in front alone; the
    batch in reverse order gives the outputs in reverse order, bit for bit."""
    form, N, L, A, _ = c
    inp = _ref(c, kind)[0]
    HD, Lp = A * D, AR.pitch(form, L)
    d = device_inputs(inp, kind)
    _, full = twice(lambda: launch(form, kind, d, N, L, A))
    per_seq = dict(ctx=L * HD, dqkv=L * 3 * HD, bias_part=3 * HD, lse=A * Lp, delta=A * Lp)
    for n0 in range(1, N):
        got, sub = twice(lambda: launch(form, kind, d, N, L, A, n0=n0))
        assert all(got["guard"].values()), n0
        for n in sub:
            cut = n0 * per_seq[n]
            assert torch.equal(sub[n].bits().reshape(-1)[cut:], full[n].bits().reshape(-1)[cut:]), (n, n0, "sub-range bits")
            assert (sub[n].t.reshape(-1)[:cut] == SENT).all(), (n, n0, "wrote in front of its range")
    rev = lambda x: np.ascontiguousarray(x.reshape((N, -1) + x.shape[1:])[::-1]).reshape(x.shape)
    inp_r = dict(inp, qkv=rev(inp["qkv"]), dctx=rev(inp["dctx"]), mask_add=np.ascontiguousarray(inp["mask_add"][::-1]))
    d_r = device_inputs(inp_r, kind)
    _, back = twice(lambda: launch(form, kind, d_r, N, L, A))
    for n in back:
        a = full[n].bits().reshape(N, -1)
        assert torch.equal(back[n].bits().reshape(N, -1), torch.flip(a, [0])), (n, "reversed batch")


# ------------------------------------------------------------------------------------------------ argument checks
@pytest.mark.parametrize("kind", RR.KINDS)
def test_attention_rejects_bad_arguments(kind):
    """Every one of these returns TNR_EINVAL before any launch: L = 0, L = 33 (l32) / 513 (long), a null pointer, a 16-bit pointer
    that is not 16-byte aligned (the kernels load and store 16-byte vectors).  No output is written."""
    td, sfx = RR.tdtype(kind), RR.SFX[kind]
    N, L, A = 2, 8, 1
    x16 = torch.zeros((N * 64, 3 * D), device=DEV, dtype=td)
    f32 = torch.zeros((N * 64 * 64,), device=DEV)
    o16, o32 = Buf(N * 64, 3 * D, dtype=td), Buf(N * 64)
    odd = lambda t: t.data_ptr() + 2
    l32f = lambda l=L, qkv=x16, ctx=o16.t: ("tnr_attn_l32_fwd" + sfx, qkv, f32, f32, ctx, N, l, A)
    l32b = lambda l=L, qkv=x16, dctx=x16, dqkv=o16.t: ("tnr_attn_l32_bwd" + sfx, qkv, f32, f32, dctx, dqkv, o32.t, N, l, A)
    lngf = lambda l=L, qkv=x16, ctx=o16.t, lse=o32.t: ("tnr_attn_long_fwd" + sfx, qkv, f32, f32, ctx, lse, N, l, A)
    lngb = lambda l=L, qkv=x16, ctx=x16, dctx=x16, dqkv=o16.t, lse=f32: ("tnr_attn_long_bwd" + sfx, qkv, f32, f32, ctx, dctx, lse, o32.t, dqkv, N, l, A)
    bad = [("l32 fwd L = 0", l32f(0), "1<=L<=32"), ("l32 fwd L = 33", l32f(33), "1<=L<=32"), ("l32 bwd L = 0", l32b(0), "1<=L<=32"),
           ("l32 bwd L = 33", l32b(33), "1<=L<=32"), ("long fwd L = 0", lngf(0), "1<=L<=512"), ("long fwd L = 513", lngf(513), "1<=L<=512"),
           ("long bwd L = 0", lngb(0), "1<=L<=512"), ("long bwd L = 513", lngb(513), "1<=L<=512"),
           ("l32 fwd null qkv", l32f(qkv=None), "null pointer"), ("l32 fwd null ctx", l32f(ctx=None), "null pointer"),
           ("l32 bwd null dctx", l32b(dctx=None), "null pointer"), ("l32 bwd null dqkv", l32b(dqkv=None), "null pointer"),
           ("long fwd null lse", lngf(lse=None), "null pointer"), ("long fwd null qkv", lngf(qkv=None), "null pointer"),
           ("long bwd null ctx", lngb(ctx=None), "null pointer"), ("long bwd null lse", lngb(lse=None), "null pointer"),
           ("l32 fwd qkv + 2", l32f(qkv=odd(x16)), "16-byte alignment"), ("l32 fwd ctx + 2", l32f(ctx=odd(o16.t)), "16-byte alignment"),
           ("l32 bwd qkv + 2", l32b(qkv=odd(x16)), "16-byte alignment"), ("l32 bwd dctx + 2", l32b(dctx=odd(x16)), "16-byte alignment"),
           ("l32 bwd dqkv + 2", l32b(dqkv=odd(o16.t)), "16-byte alignment"),
           ("long fwd qkv + 2", lngf(qkv=odd(x16)), "16-byte alignment"), ("long fwd ctx + 2", lngf(ctx=odd(o16.t)), "16-byte alignment"),
           ("long bwd qkv + 2", lngb(qkv=odd(x16)), "16-byte alignment"), ("long bwd ctx + 2", lngb(ctx=odd(x16)), "16-byte alignment"),
           ("long bwd dctx + 2", lngb(dctx=odd(x16)), "16-byte alignment"), ("long bwd dqkv + 2", lngb(dqkv=odd(o16.t)), "16-byte alignment")]
    for what, args, word in bad:
        with pytest.raises(T.TnrError) as ei:
            T.call(*args)
        msg = str(ei.value)
        assert "failed (-1)" in msg and word in msg.split("): ", 1)[1], what + ": refused for another reason: " + msg
    torch.cuda.synchronize()
    for buf in (o16, o32):
        assert (buf.raw == SENT).all(), "a refused call wrote to an output"
