"""GPU: train_embeddings=True under every optimiser option and every form of the step.

The model, feeds and weights are those of tests/history_ref.py with train_embeddings=True (hidden 256, two layers, layer 1 trainable
over a frozen layer 0 that only passes the gradient on; vocab 2000, max_pos 128: the word table is 512 000 elements, 125 LAMB chunks).
The three embedding tables and the embedding LayerNorm lie at offset 0 of flat[True] / flat_g and form the gradient bucket that
completes last.  The drivers and float64 references are those of tests/test_step_history_gpu.py, test_grad_clip_gpu.py,
test_adamw_gpu.py, test_ema_gpu.py, test_lamb_gpu.py, test_resume_gpu.py and test_variants_gpu.py, run on this layout; every bound is
one of theirs and is named where it is applied.

Gradients written with fill() get the embedding block's real sparsity (_sfill): zeros outside the parameters' slots, on every word
row the feed SPARSE does not name, row 0 (the padding row) among them, on the position rows from num_words on and on token-type
row 1, as Engine._embed_bwd leaves them (it never writes those position and token-type rows, which no token reaches: a value
written there would outlive every later backward).
The float64 references read that flat_g back from the device, so both sides see the same bits."""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import adamw_ref as A                                            # noqa: E402
import clip_ref as C                                             # noqa: E402
import ema_ref as M                                              # noqa: E402
import engine as E                                               # noqa: E402
import history_ref as HR                                         # noqa: E402
import lamb_ref as L                                             # noqa: E402
import variants_ref as V                                         # noqa: E402
from embed_train_ref import EMB_KEYS, WORD                       # noqa: E402
from test_step_history_gpu import DEV, _engine, _run, _shared, _t                       # noqa: E402
from test_grad_clip_gpu import FakeSync, fill, gen, state        # noqa: E402
from test_adamw_gpu import GS, ON, RATES, TD, WD, W as WARM, compare, ref_state, tables     # noqa: E402
from test_ema_gpu import DECAY, STEP, compare_ema, full_state, misses                   # noqa: E402
import test_lamb_gpu as TL                                       # noqa: E402
from test_resume_gpu import drain, host, same, scaler_fields     # noqa: E402

SPARSE = "full_a"                      # the feed whose word rows a fill()ed gradient keeps: 774 of 2 000 rows
LN_KEYS = tuple(EMB_KEYS[3:])          # embeddings.LayerNorm.weight / .bias
_MASKS = {}


def _emb(dtype, B=2, **more):
    eng = _engine(dtype, B, train_embeddings=True, **more)
    eng.load_state_dict(_shared()["P"])
    assert eng.lo == 0 and set(EMB_KEYS) <= set(eng.grads) and eng.off(WORD) == 0
    return eng


def _emb_elements(eng):
    """bool[n_train]: the elements of the five embedding parameters."""
    m = np.zeros(eng.n_train, bool)
    for k in EMB_KEYS:
        _, o, n, _ = eng.slot[k]
        m[o:o + n] = True
    return m


def _masks(eng):
    """Device masks of the layout, made once: what lies outside the slots, the word rows SPARSE does not name, and the count of the
    elements _sfill leaves non-zero."""
    if "out" not in _MASKS:
        rows = np.ones(HR.VOCAB, bool)
        rows[HR.named_tokens(HR.step(SPARSE))] = False
        assert rows[0] and rows.sum() > HR.VOCAB // 2
        _MASKS.update(out=torch.from_numpy(~V.slot_mask(eng.slot, eng.n_train)).to(DEV), rows=torch.from_numpy(rows).to(DEV),
                      n_in=int(V.slot_mask(eng.slot, eng.n_train).sum()) -
                      (int(rows.sum()) + HR.MAX_POS - HR.L + eng.slot[EMB_KEYS[2]][3][0] - 1) * HR.H)
    assert _MASKS["out"].numel() == eng.n_train
    return _MASKS


def _sfill(eng, g, scale):
    """test_grad_clip_gpu.fill, zeros outside the slots (test_variants_gpu._fill), on the word rows SPARSE does not name and on the
    position rows and the token-type row that no token of L = 17 words of type 0 reaches."""
    m = _masks(eng)
    fill(eng, g, scale)
    eng.flat_g[m["out"]] = 0.0
    eng.grad(EMB_KEYS[1])[HR.L:] = 0.0
    eng.grad(EMB_KEYS[2])[1:] = 0.0
    gw = eng.grad(WORD)
    gw[m["rows"]] = 0.0
    assert int(m["rows"].sum()) > gw.shape[0] // 2 and float(gw[m["rows"]].abs().max()) == 0.0
    assert float(gw[~m["rows"]].abs().max(1).values.min()) > 0.0


def _everything(eng):
    """test_variants_gpu._everything with the count of the elements _sfill leaves non-zero: decay 0.01, W = 2, T = 5, a threshold of
    0.6 of the expected norm of a 1e-3 fill (it clips), the average."""
    return dict(ON, max_grad_norm=0.6 * GS * 1e-3 * float(np.sqrt(_masks(eng)["n_in"])), ema_decay=DECAY)


def _differ(eng, a, b):
    """Where two buffers laid out like flat[True] differ: [(key or "outside the slots", elements)]."""
    ne = (a != b)
    out = [(k, int(ne[o:o + n].sum())) for k, (tr, o, n, _) in eng.slot.items() if tr and bool(ne[o:o + n].any())]
    gaps = int(ne[_masks(eng)["out"]].sum())
    return out + ([("outside the slots", gaps)] if gaps else [])


def _zero_rows(eng, t):
    """The rows of a (vocab, H) view at the word table's place in buffer t that SPARSE does not name."""
    _, o, n, shp = eng.slot[WORD]
    return t[o:o + n].view(shp)[_masks(eng)["rows"]]


# ---------------------------------------------------------------------------------------------------------------- 1: layout
@pytest.mark.parametrize("vocab,max_pos", [(HR.VOCAB, HR.MAX_POS), (30522, 512)])
def test_layout_tables_with_the_embedding_block(vocab, max_pos):
    """The history model and the same model with the shipped table sizes (7.8 M word elements; one engine, no step), the assertions
    of test_bucket_ranges_and_decay_map_tile_the_flat_buffer (tests/test_variants_gpu.py) and of tests/test_lamb_cpu.py on the
    engine's own tables: bucket_ranges() tile [0, n_train), the embedding bucket is last and starts at 0, no parameter straddles
    two buckets; decay_words == the name-derived variants_ref.decay_table (the three tables set, the embedding LayerNorm and every
    gap clear) == _decay_bits() read back; lamb_ref.check_chunks on lamb_chunks(), the device copies equal the host tables, the
    word table in ceil(n / 4096) chunks of which only the last may be partial."""
    cfg = E.EngineConfig(**dict(HR.engine_kwargs(), vocab=vocab, max_pos=max_pos), train_embeddings=True)
    eng = E.Engine(cfg, DEV, max_batch=2, dtype="fp16")
    n = eng.n_train
    ranges = eng.bucket_ranges()
    br = sorted(ranges)
    assert br[0][0] == 0 and br[-1][1] == n == eng.flat_g.numel() and all(a[1] == b[0] for a, b in zip(br, br[1:]))
    last = EMB_KEYS[-1]
    assert ranges[-1] == br[0] and ranges[-1][0] == eng.off(WORD) == 0 and len(ranges) == 4
    assert ranges[-1][1] == (eng.off(last) + eng.slot[last][2] + 63) // 64 * 64
    assert all(ranges[-1][0] <= eng.off(k) and eng.off(k) + eng.slot[k][2] <= ranges[-1][1] for k in EMB_KEYS)
    assert eng.slot[WORD][2] == vocab * HR.H and eng.slot[EMB_KEYS[1]][2] == max_pos * HR.H
    mask, inside = V.decay_table(eng.slot, n), V.slot_mask(eng.slot, n)
    words = E.decay_words(eng.slot, n)
    bits = np.unpackbits(words.view(np.uint8), bitorder="little").astype(bool)
    assert words.size == (n + 31) // 32 and np.array_equal(bits[:n], mask) and not bits[n:].any()
    covered = np.zeros(n, bool)
    for k, (tr, o, cnt, shp) in eng.slot.items():
        if tr:
            assert not covered[o:o + cnt].any() and cnt == int(np.prod(shp)), k
            covered[o:o + cnt] = True
            assert any(s <= o and o + cnt <= e for s, e in br), k
    assert np.array_equal(covered, inside) and not mask[~inside].any()
    for k in EMB_KEYS:
        _, o, cnt, _ = eng.slot[k]
        assert mask[o:o + cnt].all() if k in EMB_KEYS[:3] else not mask[o:o + cnt].any(), k
    assert mask.sum() == sum(cnt for k, (tr, o, cnt, shp) in eng.slot.items() if tr and A.decays(k, shp))
    assert np.array_equal(A.unpack(eng._decay_bits().cpu().numpy(), n), mask)
    names, chunks, tensors = E.lamb_chunks(eng.slot, n)
    L.check_chunks(L.slots(eng.slot), n, chunks, tensors, names)
    ls = eng._lamb_buffers()
    assert ls.names == names and np.array_equal(ls.chunks.cpu().numpy(), chunks) and np.array_equal(ls.tensors.cpu().numpy(), tensors)
    assert np.array_equal(ls.chunks_host.numpy(), chunks) and np.array_equal(ls.tensors_host.numpy(), tensors)
    assert names[0] == WORD and set(names) == {k for k, s_ in eng.slot.items() if s_[0]}
    fc, nc, adapted, _ = tensors[0].tolist()
    nw = vocab * HR.H
    assert (fc, nc, adapted) == (0, -(-nw // L.CHUNK), 1) and (chunks[:nc - 1, 1] == L.CHUNK).all()
    assert chunks[nc - 1, 1] == nw - (nc - 1) * L.CHUNK and (chunks[:nc, 2] == 0).all() and nc == (125 if vocab == HR.VOCAB else 1908)
    assert [int(tensors[names.index(k), 2]) for k in EMB_KEYS] == [1, 1, 1, 0, 0]


# ---------------------------------------------------------------------------------------------------------------- 2: AdamW family
def _ref_step(ref, e, gh, s, lr, mask, coef, wd=WD, w=1.0 - DECAY, gs=GS):
    """One float64 step of test_three_optimiser_steps_against_float64's driver: s updates precede it."""
    mult = A.schedule(s, WARM, TD)
    *ref, e = M.adamw_ema_step(ref[0], gh, ref[1], ref[2], ref[3], e, s + 1, lr * mult, mask, wd, w, grad_scale=gs * coef)
    return ref, e


@pytest.mark.parametrize("dtype,ams", [("fp16", True), ("bf16", False)])
def test_three_adamw_steps_against_float64(dtype, ams):
    """The body of test_three_optimiser_steps_against_float64 (tests/test_variants_gpu.py) with the embeddings trainable and the word
    gradient sparse: three rates (lr 2e-2, lr_bert 1e-2, lr_news_head 5e-3), weight decay 0.01, clipping (which clips steps 1 and
    3), the schedule W = 2, T = 5 and ema_decay 0.9 against ema_ref.adamw_ema_step / adamw_ref.schedule / clip_ref.clip in float64,
    rates and decay mask from parameter NAMES (variants_ref.rate_table / decay_table: `.bert_model.` -> lr_bert, which the
    embedding keys carry).  Bounds of test_three_steps_against_float64 (tests/test_adamw_gpu.py, test_ema_gpu.py): p and the
    average rtol 1e-5 atol 1e-6; m, v, vmax rtol 1e-5 with a floor of 1e-5 of the buffer's largest magnitude.
    The same float64 run in which only the embedding block's elements get lr instead of lr_bert misses the engine's parameters in
    more than 99 % of those elements and in none outside them.
    Under decay a zero-gradient word row, row 0 included, moves by the decay factor only - p (1 - lr_bert mult wd) per step, m = v
    = 0 - as torch.optim.AdamW moves every row of a dense embedding gradient; that is part of the float64 comparison above, which
    covers every element.  A fourth step with weight_decay = 0 and no average: those rows keep their bits, and their m, v, vmax
    are exactly 0."""
    eng = _emb(dtype)
    n = eng.n_train
    lr, mask = V.rate_table(eng.slot, n, RATES), V.decay_table(eng.slot, n)
    emb = _emb_elements(eng)
    assert (lr[emb] == RATES[1]).all() and emb[:eng.bucket_ranges()[-1][1]].sum() == emb.sum() > 500000
    lr_alt = np.where(emb, RATES[0], lr)
    kw = _everything(eng)
    ref, alt = ref_state(eng, ams), ref_state(eng, ams)
    p0 = ref[0].copy()
    e = e_alt = p0.copy()
    g = gen()
    for s, sc in enumerate((1e-3, 1e-4, 1e-3)):
        _sfill(eng, g, sc)
        gh = eng.flat_g.cpu().numpy()
        eng.step(RATES[0], amsgrad=ams, **STEP, **kw)
        assert eng.lr_scale == A.schedule(s, WARM, TD) == (0.0, 0.5, 1.0)[s]
        coef = C.clip([gh], kw["max_grad_norm"], GS)[1]
        assert (coef < 1.0) == (s != 1), (s, coef)                       # steps 1 and 3 are clipped, the small one is not
        ref, e = _ref_step(ref, e, gh, s, lr, mask, coef)
        alt, e_alt = _ref_step(alt, e_alt, gh, s, lr_alt, mask, coef)
        what = "embed steps %s ams%d step%d" % (dtype, ams, s + 1)
        compare(what, eng, ref, ams)
        compare_ema(what, eng, e)
        if s == 0:
            assert torch.equal(eng._ema, eng.flat[True])                   # rate 0: p kept its bits
    assert misses(eng, ref[0]) and misses(eng, p0) and eng.ema_updates == 3
    got = eng.flat[True].cpu().numpy().astype(np.float64)
    over = np.abs(got - alt[0]) > 1e-6 + 1e-5 * np.abs(alt[0])
    print("\n[embed steps %s] lr for lr_bert on the embedding block: misses %.4f of its elements, %d outside" % (
        dtype, over[emb].mean(), int(over[~emb].sum())))
    assert not over[~emb].any() and over[emb].mean() > 0.99, (int(over[~emb].sum()), float(over[emb].mean()))
    assert np.array_equal(A.unpack(eng._decay_map.cpu().numpy(), n), mask)
    rows0 = _zero_rows(eng, eng.flat[True]).clone()
    assert not torch.equal(rows0, _zero_rows(eng, _t(p0.astype(np.float32))))                  # the decay did move them
    _sfill(eng, g, 1e-3)
    eng.step(RATES[0], amsgrad=ams, **STEP, **dict(kw, weight_decay=0.0, ema_decay=None))
    torch.cuda.synchronize()
    assert torch.equal(rows0, _zero_rows(eng, eng.flat[True])) and rows0.shape[0] > HR.VOCAB // 2
    for buf in (eng.adam_m, eng.adam_v, eng.adam_vmax):
        assert float(_zero_rows(eng, buf).abs().max()) == 0.0
    assert float(eng.adam_m[:eng.slot[WORD][2]].abs().max()) > 0.0
    if dtype == "fp16":
        eng.scaler.drain(eng)
        assert eng.scaler.skipped == 0 and eng.step_count == 4


# ---------------------------------------------------------------------------------------------------------------- 3: LAMB
@pytest.mark.parametrize("extras", [False, True], ids=["plain", "clip_ema"])
@pytest.mark.parametrize("dtype,ams", [("fp16", True), ("bf16", False)])
def test_three_lamb_steps_against_float64(dtype, ams, extras):
    """The body of test_three_steps_against_float64 (tests/test_lamb_gpu.py): every step against lamb_ref.lamb_step from the engine's
    own state before it, with its bounds (p and the average rtol 1e-5 atol 1e-6; m, v, vmax rtol 1e-5 with a floor of 1e-5 of the
    buffer's largest magnitude; trust within lamb_ref.trust_rtol(kappa), whose precondition trust_rtol(kappa) < 1e-5 for every
    adapted tensor compare_trust asserts).  trust_ratios() names the three tables and not the embedding LayerNorm."""
    eng = _emb(dtype)
    n = eng.n_train
    inside = V.slot_mask(eng.slot, n)
    assert np.array_equal(tables(eng, RATES)[0][inside], V.rate_table(eng.slot, n, RATES)[inside])     # test_lamb_gpu.expected's rates
    max_norm = _everything(eng)["max_grad_norm"]
    kw = dict(TL.ON, **(dict(max_grad_norm=max_norm, ema_decay=0.9) if extras else {}))
    p0 = eng.flat[True].clone()
    g, coefs, kappa = gen(), [], 0.0
    for s, sc in enumerate((1e-3, 1e-4, 1e-3)):
        _sfill(eng, g, sc)
        gh = eng.flat_g.cpu().numpy()
        pre = TL.snapshot(eng, ams, extras)
        eng.step(RATES[0], amsgrad=ams, **TL.RKW, **kw)
        mult = A.schedule(s, WARM, TD)
        assert eng.lr_scale == mult == (0.0, 0.5, 1.0)[s]
        coef = eng.grad_norm()[1] if extras else None
        coefs.append(coef)
        want = TL.expected(eng, pre, gh, s + 1, mult, ams, coef=coef, ema_w=1.0 - 0.9 if extras else None)
        TL.compare("embed lamb %s ams%d extras%d step%d" % (dtype, ams, extras, s + 1), eng, want, ams)
        kappa = max(kappa, max(want["info"][k][3] for k in eng.trust_ratios()))
        if s == 0:
            assert torch.equal(eng.flat[True], p0) and (not extras or torch.equal(eng._ema, p0))
    got = eng.trust_ratios()
    assert set(EMB_KEYS[:3]) <= set(got) and not (set(LN_KEYS) & set(got))
    print("[embed lamb %s extras%d] largest kappa of an adapted tensor %.3f (trust_rtol %.2e); word table trust %.4g" % (
        dtype, extras, kappa, L.trust_rtol(kappa), got[WORD][0]))
    if extras:
        assert coefs[0] < 1.0 and coefs[1] == 1.0 and coefs[2] < 1.0
    TL.adam_misses_adapted_only(eng, pre, gh, 3, 1.0, ams, coef)
    assert eng._decay_map is None
    if dtype == "fp16":
        eng.scaler.drain(eng)
        assert eng.scaler.skipped == 0 and eng.step_count == 3


# ---------------------------------------------------------------------------------------------------------------- 4: bucketed
MODES = {"fp16_everything": ("fp16", lambda eng: _everything(eng)),
         "bf16_clip": ("bf16", lambda eng: dict(max_grad_norm=_everything(eng)["max_grad_norm"], ema_decay=DECAY)),
         "bf16_by_bucket": ("bf16", lambda eng: dict(ON, ema_decay=DECAY)),
         "fp16_lamb": ("fp16", lambda eng: dict(_everything(eng), lamb=True)),
         "bf16_lamb": ("bf16", lambda eng: dict(ON, lamb=True, ema_decay=DECAY))}


@pytest.mark.parametrize("mode", list(MODES))
def test_bucketed_step_equals_the_whole_one(mode, monkeypatch):
    """As test_bucketed_equals_whole (tests/test_adamw_gpu.py, test_ema_gpu.py, test_lamb_gpu.py): a FakeSync over bucket_ranges()
    against no sync, three steps, bit for bit in parameters, moments, a 16-bit weight copy, the average (and the trust table), the
    buckets waited for in completion order, each once.  bf16_by_bucket has nothing that needs the whole gradient: Engine.step
    updates bucket by bucket, its last bucket lies at offset 0, and the loop over what lies outside the buckets must not reach
    it again - every launch of that mode is recorded and the launches must tile [0, n_train) exactly once."""
    import tnr_hip as T
    dtype, kw_of = MODES[mode]
    outs, trusts = [], []
    for how in ("whole", "bucketed"):
        eng = _emb(dtype)
        p0 = eng.flat[True].clone()
        g, ranges, kw = gen(), eng.bucket_ranges(), kw_of(eng)
        for step in range(3):
            _sfill(eng, g, 1e-3)
            sync = FakeSync(ranges) if how == "bucketed" else None
            spans = []
            if mode == "bf16_by_bucket" and sync is not None:
                real, base = T.call, eng.flat[True].data_ptr()

                def recorder(name, *a, real=real, base=base):
                    if name == "tnr_adamw_step_ema":
                        spans.append(((a[0].data_ptr() - base) // 4, a[5]))
                    return real(name, *a)
                monkeypatch.setattr(T, "call", recorder)
            eng.step(RATES[0], amsgrad=dtype == "fp16", sync=sync, ema_warmup=True, **STEP, **kw)
            monkeypatch.undo()
            if sync is not None:
                assert sync.waited == list(range(len(ranges))) and not sync.pending
            if spans:
                cover = np.zeros(eng.n_train, np.int64)
                for o, cnt in spans:
                    cover[o:o + cnt] += 1
                assert (cover == 1).all() and spans[-1][0] + spans[-1][1] <= ranges[-1][1], "the bucket-by-bucket launches do not tile flat[True] once"
        outs.append(full_state(eng) + ([eng._lamb_state.trust.clone()] if "lamb" in mode else []))
        trusts.append(eng.trust_ratios())
        if dtype == "fp16":
            eng.scaler.drain(eng)
            assert eng.scaler.skipped == 0
    assert len(outs[0]) == (7 if "lamb" in mode else 6) and all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(*outs))
    assert trusts[0] == trusts[1] and (trusts[0] is not None) == ("lamb" in mode)
    assert not torch.equal(outs[0][5], p0) and not torch.equal(outs[0][5], outs[0][0])
    o, cnt = eng.slot[WORD][1:3]
    assert not torch.equal(outs[0][0][o:o + cnt], p0[o:o + cnt])


# ---------------------------------------------------------------------------------------------------------------- 5: accumulation
_PLAIN = {}


def _plain(dtype):
    """Plain backwards of full_a and full_b on one engine, full_b once more under a no-op bucket hook; flat_g cloned (the rule of
    tests/test_grad_accum_gpu.plain).  Computed once per type, never modified."""
    if dtype not in _PLAIN:
        eng = _emb(dtype, HR.B_FULL)
        ga = _run(eng, HR.step("full_a"))["flat_g"]
        gb = _run(eng, HR.step("full_b"))["flat_g"]
        gbh = _run(eng, HR.step("full_b", hook=True))["flat_g"]
        torch.cuda.synchronize()
        _PLAIN[dtype] = dict(a=ga, b=gb, total=ga + gb, total_hooked=ga + gbh)
    return _PLAIN[dtype]


@pytest.mark.parametrize("hook", [False, True])
@pytest.mark.parametrize("dtype,ams", [("fp16", True), ("bf16", False)])
def test_accumulation_window_with_the_embedding_bucket(dtype, ams, hook):
    """full_a and full_b as micro-batches (0, 2) and (1, 2): flat_g after the window is g_a + g_b of two plain backwards, bit for bit
    (torch's fp32 `+` is the reference: tests/test_grad_accum_gpu.py); under a hook every bucket holds the sum when its hook
    fires, once per bucket, the embedding bucket last.  Word rows only full_a names hold that feed's single-batch bits, rows
    neither names are exactly zero.  Then two step(grad_scale = 0.5, everything on) on the window's gradient (the update does not
    consume it; the first has rate 0) against the float64 driver of test_three_adamw_steps_against_float64 with its bounds."""
    ref = _plain(dtype)
    eng = _emb(dtype, HR.B_FULL)
    ranges = eng.bucket_ranges()
    fired, clones = [], []

    def after(b):
        fired.append(b)
        clones.append(eng.flat_g[ranges[b][0]:ranges[b][1]].clone())
    s = _shared()
    for j, fid in enumerate(("full_a", "full_b")):
        if not hook:
            _run(eng, HR.step(fid, micro=(j, 2)))
            continue
        h, m, c, y = (_t(x) for x in HR.feed(fid))         # _run's own hook expects every bucket to fire in every backward
        eng.forward_indexed(s["comb"], h, m, c, y, s["tables"])
        eng.backward(after_bucket=after, micro=(j, 2))
        assert fired == ([] if j == 0 else list(range(len(ranges))))          # no collective starts inside the window
    torch.cuda.synchronize()
    assert eng._acc_held == 0
    total = ref["total_hooked"] if hook else ref["total"]
    assert torch.equal(eng.flat_g.view(torch.int32), total.view(torch.int32)) and not torch.equal(eng.flat_g, ref["b"])
    if hook:
        assert fired == list(range(len(ranges))) and fired[-1] == len(ranges) - 1 and ranges[-1][0] == eng.off(WORD)
        for b, (s_, e_) in enumerate(ranges):
            assert torch.equal(clones[b], total[s_:e_]), "bucket %d did not hold the window's sum when its hook fired" % b
    na, nb = HR.named_tokens(HR.step("full_a")), HR.named_tokens(HR.step("full_b"))
    only_a, neither = np.setdiff1d(na, nb), np.setdiff1d(np.arange(HR.VOCAB), np.union1d(na, nb))
    assert only_a.size > 100 and neither.size > 1000 and 0 in neither
    gw, ga = eng.grad(WORD), ref["a"][:eng.slot[WORD][2]].view(eng.slot[WORD][3])
    assert torch.equal(gw[_t(only_a)], ga[_t(only_a)]) and float(gw[_t(only_a)].abs().max(1).values.min()) > 0.0
    assert float(gw[_t(neither)].abs().max()) == 0.0
    assert float(gw[_t(np.union1d(na, nb))].abs().max(1).values.min()) > 0.0
    # the step on the window's sum
    n = eng.n_train
    lr, mask = V.rate_table(eng.slot, n, RATES), V.decay_table(eng.slot, n)
    gh = eng.flat_g.cpu().numpy()
    max_norm = 0.5 * 0.5 * float(np.sqrt((gh.astype(np.float64) ** 2).sum()))          # half the mean gradient's norm: it clips
    kw = dict(ON, max_grad_norm=max_norm, ema_decay=DECAY, grad_scale=0.5, lr_bert=RATES[1], lr_news_head=RATES[2])
    st = ref_state(eng, ams)
    e = st[0].copy()
    for s in range(2):
        eng.step(RATES[0], amsgrad=ams, **kw)
        coef = C.clip([gh], max_norm, 0.5)[1]
        assert coef < 0.75
        st, e = _ref_step(st, e, gh, s, lr, mask, coef, gs=0.5)
        what = "embed window %s hook%d step%d" % (dtype, hook, s + 1)
        compare(what, eng, st, ams)
        compare_ema(what, eng, e)
    assert misses(eng, st[0]) and eng.ema_updates == 2
    if dtype == "fp16":
        eng.scaler.drain(eng)
        assert eng.scaler.skipped == 0 and eng.step_count == 2


# ---------------------------------------------------------------------------------------------------------------- 6: overflow
def _copies(eng):
    return [t.clone() for d in eng.sh for t in d.values()] + [eng.sh_a1.clone(), eng.sh_a1T.clone()]


def _opt_state(eng):
    torch.cuda.synchronize()
    out = state(eng)[:4] + [eng._clip_owner._ema.clone()]
    return out + ([eng._lamb_state.trust.clone()] if eng._lamb_state is not None else [])


@pytest.mark.parametrize("where", ["flat_g", "accumulator"])
@pytest.mark.parametrize("opt", ["adamw", "lamb"])
def test_fp16_overflow_in_the_embedding_block_skips_the_whole_update(opt, where):
    """fp16 at the short batch, real backwards, everything on (AdamW + average, or LAMB + average): one clean step, then a step whose
    gradient holds an inf in a word row the step names - written into flat_g before step(), or into the accumulator's embedding
    region after micro-batch 0 of a window of two, as test_fp16_overflow_in_a_micro_batch_under_nrms_skips_the_whole_update
    (tests/test_variants_gpu.py) does.  Parameters, m, v, vmax, the average, the trust table and every 16-bit copy keep their bits;
    one step is counted as skipped, step_count is corrected and the multiplier is 0.5; the next clean step equals, bit for bit, the
    step of an engine that never overflowed and runs at that multiplier."""
    lamb = opt == "lamb"
    row = int(HR.named_tokens(HR.step("short_b"))[3])

    def kw_of(eng):
        return dict(_everything(eng), grad_scale=0.5 if where == "accumulator" else 1.0, lr_bert=RATES[1], lr_news_head=RATES[2],
                    **(dict(lamb=True) if lamb else {}))

    def clean(eng, fids):
        if where == "accumulator":
            for j, fid in enumerate(fids):
                _run(eng, HR.step(fid, micro=(j, 2)))
        else:
            _run(eng, HR.step(fids[0]))
        eng.step(RATES[0], **kw_of(eng))

    eng = _emb("fp16", HR.B_SHORT)
    clean(eng, ("short_a", "short_b"))
    clean(eng, ("short_a", "short_b"))                                    # the second update of the warm-up: the parameters move
    eng.scaler.drain(eng)
    assert eng.scaler.skipped == 0 and eng.step_count == 2
    spot = eng.off(WORD) + row * HR.H + 5
    if where == "accumulator":
        _run(eng, HR.step("short_b", micro=(0, 2)))
        assert float(eng._acc[spot].abs()) > 0.0
        eng._acc[spot] = float("inf")                                     # as if micro-batch 0's backward had overflowed in that row
        _run(eng, HR.step("short_a", micro=(1, 2)))
    else:
        _run(eng, HR.step("short_b"))
        assert float(eng.flat_g[spot].abs()) > 0.0
        eng.flat_g[spot] = float("inf")
    before, sh = _opt_state(eng), _copies(eng)
    assert not bool(torch.isfinite(eng.flat_g).all()) and eng._acc_held == 0 and len(before) == (6 if lamb else 5)
    trust = eng.trust_ratios()
    eng.step(RATES[0], **kw_of(eng))
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(before, _opt_state(eng)))
    assert all(torch.equal(a, b) for a, b in zip(sh, _copies(eng))) and eng.trust_ratios() == trust
    eng.scaler.drain(eng)
    assert eng.scaler.skipped == 1 and eng.step_count == 2 and eng.scaler.mult == 0.5 and eng.ema_updates == 2
    other = _emb("fp16", HR.B_SHORT)
    clean(other, ("short_a", "short_b"))
    clean(other, ("short_a", "short_b"))
    other.scaler.drain(other)
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(before, _opt_state(other)))
    other.scaler.mult = eng.scaler.mult
    for e_ in (eng, other):
        clean(e_, ("short_b", "short_a"))
        e_.scaler.drain(e_)
    assert torch.equal(eng.flat_g, other.flat_g) and bool(torch.isfinite(eng.flat_g).all())
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(_opt_state(eng), _opt_state(other)))
    assert all(torch.equal(a, b) for a, b in zip(_copies(eng), _copies(other))) and eng.trust_ratios() == other.trust_ratios()
    assert (eng.scaler.skipped, eng.step_count, other.scaler.skipped, other.step_count) == (1, 3, 0, 3)
    assert not torch.equal(before[0], eng.flat[True]) and eng.ema_updates == other.ema_updates == 3


# ---------------------------------------------------------------------------------------------------------------- 7: checkpoint
@pytest.mark.parametrize("dtype,lamb", [("fp16", False), ("bf16", True), ("fp16", True)], ids=["fp16_adamw", "bf16_lamb", "fp16_lamb"])
def test_optimiser_checkpoint_split_equals_straight(dtype, lamb):
    """The body of test_optimiser_checkpoint_split_equals_straight (tests/test_variants_gpu.py; the rule of tests/test_resume_gpu.py)
    with everything on, AdamW + average or LAMB + average: three steps on written gradients, optimizer_state_dict(), a fresh engine,
    load_state_dict + load_ema_state_dict + load_optimizer_state_dict, then two real forward / backward steps on feeds - the
    forward reads the restored tables - torch.equal to five straight steps in parameters, moments, a 16-bit weight copy, the
    average and the scaler fields.  The saved state lists exactly the trainable keys in slot order, the five embedding keys among
    them, and ema_state_dict() holds their averages."""
    def run(eng, steps, kw):
        for s in steps:
            if s < 3:
                _sfill(eng, torch.Generator(device=DEV).manual_seed(100 + s), 1e-3)
            else:
                _run(eng, HR.step(("short_a", "short_b")[s - 3], form=("idx", "tok")[s - 3]))
            eng.step(RATES[0], amsgrad=dtype == "fp16", **STEP, **kw)

    straight = _emb(dtype, HR.B_SHORT)
    kw = dict(_everything(straight), **(dict(lamb=True) if lamb else {}))
    run(straight, range(3), kw)
    drain(straight)
    run(straight, range(3, 5), kw)
    first = _emb(dtype, HR.B_SHORT)
    run(first, range(3), kw)
    sd, esd, osd = host(first.state_dict()), host(first.ema_state_dict()), first.optimizer_state_dict()
    trainable = [k for k, s_ in first.slot.items() if s_[0]]
    assert osd["step"] == 3 and osd["ema_updates"] == 3 and list(osd["state"]) == trainable and set(EMB_KEYS) <= set(trainable)
    assert trainable[:5] == list(EMB_KEYS) and set(esd) == set(sd) and set(EMB_KEYS) <= set(esd)
    for k in EMB_KEYS:
        _, o, cnt, shp = first.slot[k]
        assert torch.equal(esd[k].reshape(-1), first._ema[o:o + cnt].cpu()) and not torch.equal(esd[k], sd[k]), k
        assert all(tuple(t.shape) == tuple(shp) and float(t.abs().max()) > 0.0 for n_, t in osd["state"][k].items()
                   if dtype == "fp16" or n_ != "max_exp_avg_sq"), k
    del first
    second = _engine(dtype, HR.B_SHORT, train_embeddings=True)
    second.load_state_dict(sd)
    second.load_ema_state_dict(esd)
    second.load_optimizer_state_dict(osd)
    assert second.step_count == 3
    run(second, range(3, 5), kw)
    assert torch.equal(straight.flat_g, second.flat_g), _differ(second, straight.flat_g, second.flat_g)
    assert torch.equal(straight.flat[True], second.flat[True]), _differ(second, straight.flat[True], second.flat[True])
    assert same(full_state(straight), full_state(second)) and len(full_state(second)) == 6
    drain(straight)
    drain(second)
    assert second.step_count == straight.step_count == 5 and scaler_fields(second) == scaler_fields(straight)
    assert second.ema_updates == straight.ema_updates == 5 and second.lr_scale == straight.lr_scale
    assert second.trust_ratios() == straight.trust_ratios() and (second.trust_ratios() is not None) == lamb
    fresh = _emb(dtype, HR.B_SHORT)
    assert not torch.equal(second.flat[True], fresh.flat[True]) and not torch.equal(second.p(WORD), fresh.p(WORD))
    if dtype == "fp16":
        assert straight.scaler.skipped == 0


# ---------------------------------------------------------------------------------------------------------------- 8: acc = 1
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_backward_encoder_accumulates_with_trainable_embeddings(dtype):
    """Engine._embed_bwd's accumulate branch, which no caller reaches (stage 1 refuses train_embeddings): after forward + backward
    of full_a, backward_encoder(dvec, N, acc=1) on the values of the dvec the backward handed it (a copy taken in front of the
    first pass, whose bias reduction sums dvec's columns in place).  Every accumulate path adds a FINISHED sum to what the
    gradient holds - the weight-gradient slab sum (gemm_plan.hip: s *= out_scale; s += *o), tnr_reduce_multi (dst + t), the fp32
    GEMM's beta, tnr_colsum and tnr_scatter_sum_rows (out + t) - the sums are those of the first pass in the same fixed order, and
    the scale 1 / loss scale is a power of two, so every gradient of student.news_encoder.*, the word and position tables and
    the embedding LayerNorm among them, is EXACTLY twice the first one; word rows no token names stay exactly zero; every gradient
    the encoder's backward does not write keeps its bits.
    The token-type row alone is no such sum: the first pass takes it from the L position rows, the accumulate pass from dx over
    all M rows - the same M terms in another order.  Each order is within the recursive-summation bound the kernel test uses
    (tests/test_embed_train_kernels_gpu.py: count x 2^-23 x sum |terms|) of the exact sum, and the final add rounds once:
    |g2 - 2 g1| <= 2 M 2^-23 sum |dx| + 2^-24 |g2| per column."""
    eng = _emb(dtype, HR.B_FULL)
    seen, real = {}, eng.backward_encoder

    def spy(dvec, N, *a, **k):
        assert not seen and not a and not k.get("acc")
        seen.update(dvec=dvec.clone(), N=N)
        return real(dvec, N, *a, **k)
    eng.backward_encoder = spy
    g1 = _run(eng, HR.step("full_a"))["flat_g"]
    del eng.backward_encoder
    assert seen["N"] == HR.B_FULL * (HR.U + HR.C) and float(g1.abs().max()) > 0.0
    eng.backward_encoder(seen["dvec"], seen["N"], acc=1)
    torch.cuda.synchronize()
    g2 = eng.flat_g.clone()
    TYPE = EMB_KEYS[2]
    twice, kept = [], []
    for k, (tr, o, cnt, shp) in eng.slot.items():
        if not tr:
            continue
        a, b = g1[o:o + cnt], g2[o:o + cnt]
        if k == TYPE:
            continue
        if k.startswith(E.PFX):
            assert torch.equal(b, 2.0 * a), "%s: %d elements are not twice the first pass's" % (k, int((b != 2.0 * a).sum()))
            twice.append(k)
        else:
            assert torch.equal(a, b), k
            kept.append(k)
    assert set(twice) | set(kept) | {TYPE} == set(eng.grads) and set(EMB_KEYS) - {TYPE} <= set(twice) and len(kept) >= 7
    assert all(float(g1[eng.off(k):eng.off(k) + eng.slot[k][2]].abs().max()) > 0.0 for k in EMB_KEYS)
    rows = torch.ones(HR.VOCAB, dtype=torch.bool, device=DEV)
    rows[_t(HR.named_tokens(HR.step("full_a")))] = False
    gw = eng.grad(WORD)
    assert bool(rows[0]) and float(gw[rows].abs().max()) == 0.0 and float(gw[~rows].abs().max(1).values.min()) > 0.0
    M_ = seen["N"] * HR.L
    dx = eng.dx_emb[:M_].double()
    _, o, cnt, shp = eng.slot[TYPE]
    t1, t2 = g1[o:o + cnt].view(shp).double(), g2[o:o + cnt].view(shp).double()
    bound = 2.0 * M_ * 2.0 ** -23 * dx.abs().sum(0) + 2.0 ** -24 * t2[0].abs()
    err = (t2[0] - 2.0 * t1[0]).abs()
    print("\n[embed acc=1 %s] token-type row: worst err / bound %.3e; columns where |g1| exceeds the bound %.3f" % (
        dtype, float((err / bound).max()), float((t1[0].abs() > bound).double().mean())))
    assert bool((err <= bound).all()) and float((t1[0].abs() > bound).double().mean()) > 0.9      # a pass that only wrote would miss it
    assert float(t1[1:].abs().max()) == 0.0 and float(t2[1:].abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------------------------- 9: two ranks
def test_two_ranks_equal_one_rank_with_trainable_embeddings(tmp_path):
    """The fp16 case of test_two_ranks_equal_one_rank_with_the_concatenated_batch (tests/test_dp_gpu.py) through the same worker
    (tests/workers/dp_rank.py, two processes on one GPU, then one) with train_embeddings=True at vocab 2000 / max_pos 128, clipping
    and decay on, and that test's bounds: both ranks hold identical gradients and parameters; the mean of the two half-batch
    gradients against the whole batch's within 1e-3 relative L2 in either part of the buffer; parameters after two steps within
    0.02 lr on average and 2.05 lr steps at most.  Every bucket's collective is launched once per backward, the embedding bucket's
    last, behind the embedding backward's last kernel."""
    from test_dp_gpu import WORKER
    B, steps, lr = 4, 2, 1e-4
    opts = json.dumps(dict(engine=dict(train_embeddings=True, vocab=HR.VOCAB, max_pos=HR.MAX_POS),
                           step=dict(max_grad_norm=0.02, weight_decay=0.01)))

    def launch(world, tag, port):
        out = str(tmp_path / (tag + "_rank%d.npz"))
        procs = []
        for r in range(world):
            env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
            procs.append(subprocess.Popen([sys.executable, WORKER, out, "fp16", str(B), str(steps), "stage2", opts], env=env,
                                          stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
        logs = [p.communicate(timeout=900)[0] for p in procs]
        for p, lg in zip(procs, logs):
            assert p.returncode == 0, lg[-3000:]
        return [np.load(out % r) for r in range(world)]

    t0 = time.perf_counter()
    two = launch(2, "w2", 29641)
    one = launch(1, "w1", 29642)[0]
    assert np.array_equal(two[0]["grads"], two[1]["grads"]) and np.array_equal(two[0]["params"], two[1]["params"])
    g2, g1 = two[0]["grads"][0].astype(np.float64), one["grads"][0].astype(np.float64)
    cut = int(one["head0"])
    n_emb = int(one["emb_end"])
    assert 0 < n_emb < cut and np.abs(g1[:HR.VOCAB * 768]).max() > 0.0 and (g1[:768] == 0.0).all() and (g2[:768] == 0.0).all()
    for name, sl in (("encoder + pooling", slice(0, cut)), ("heads", slice(cut, None))):
        rel = np.linalg.norm(g2[sl] - g1[sl]) / np.linalg.norm(g1[sl])
        print("embed fp16 %s: rel. L2 difference of the averaged gradient %.2e" % (name, rel))
        assert rel < 1e-3, (name, rel)
    dp = np.abs(two[0]["params"].astype(np.float64) - one["params"].astype(np.float64))
    print("embed fp16: |param diff| mean %.2e max %.2e (lr %.0e); clip (norm, coef) per step %s" % (dp.mean(), dp.max(), lr, two[0]["clip"].tolist()))
    assert dp.mean() < 0.02 * lr and dp.max() <= 2.05 * lr * steps
    assert (two[0]["clip"][:, 1] < 1.0).all() and (one["clip"][:, 1] < 1.0).all() and np.array_equal(two[0]["clip"], two[1]["clip"])
    nb = int(two[0]["n_buckets"])
    for r in two:
        assert nb == 6 and r["launched"].tolist() == list(range(nb)) * steps and bool(r["embed_then_last_launch"].all())
    assert not np.array_equal(two[0]["params"][:n_emb], one["params0"][:n_emb])
    print("embed fp16 two ranks + one rank: %.1f s" % (time.perf_counter() - t0))
