"""GPU: cls / mean pooling, the NRMS user encoder and user_log_mask under every form of the training step.

The model, feeds, plans and schedules are those of tests/history_ref.py; the variants, their weights and the name-derived rate and
decay tables are tests/variants_ref.py (pinned by tests/test_variants_ref_cpu.py):
  mean_ulm (mean, additive, user_log_mask)   cls_nrms (cls, NRMS 4 x 16)   att_nrms_ulm (att, NRMS, user_log_mask)
The drivers are the ones of tests/test_step_history_gpu.py, test_grad_clip_gpu.py, test_adamw_gpu.py, test_ema_gpu.py and
test_resume_gpu.py, taking a model.  Every bound is one the project already uses for the same comparison with attention pooling
and the additive user encoder; it is named where it is applied."""
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
import variants_ref as V                                         # noqa: E402
import widths_ref as W                                           # noqa: E402
from embed_train_ref import EMB_KEYS, WORD, rel_l2               # noqa: E402
from test_step_history_gpu import DEV, WHAT, _engine, _play, _run, _shared, _t      # noqa: E402
from test_grad_clip_gpu import FakeSync, fill, gen, state        # noqa: E402
from test_adamw_gpu import GS, ON, RATES, TD, WD, W as WARM, compare, ref_state    # noqa: E402
from test_ema_gpu import DECAY, STEP, compare_ema, full_state, misses              # noqa: E402

NRMS_KEYS = tuple(V.UE + n for n in E.NRMS_W + E.NRMS_B)


def _loaded(v, dtype, B, **more):
    eng = _engine(dtype, B, v, **more)
    eng.load_state_dict(_shared(v)["P"])
    return eng


def _against_oracle(tag, v, dtype, fid, g, eng):
    """losses, scores and every gradient of one step (a _run result) against the numpy oracle of the feed under widths_ref.TOLS -
    fp16: loss 2e-3, score 3e-3, gradients 2e-2 relative L2; bf16: 1.6e-2, 2.4e-2, 8e-2; the score relative to
    variants_ref.score_den; no-op keys below NOOP_ABS, an unused pad_doc exactly zero on both sides, no key passed over."""
    ref_l, ref_s, G, un = V.oracle(v, fid)
    ltol, stol, gtol = W.TOLS[dtype]
    le = np.abs(g["losses"][:3].cpu().numpy() - ref_l).max() / max(1.0, np.abs(ref_l).max())
    se = np.abs(g["score"].cpu().numpy() - ref_s).max() / V.score_den(v, ref_s, un)
    assert set(eng.grads) == set(G)

    def got_of(k):
        _, o, cnt, shp = eng.slot[k]
        return g["flat_g"][o:o + cnt].view(shp).cpu().numpy()
    worst, wk, bad = V.compare_grads(v, list(G), got_of, G, gtol)
    print("\n[variants %s %s %s] %s: loss %.2e score %.2e worst gradient %.2e (%s)" % (v, dtype, tag, fid, le, se, worst, wk[-48:]))
    assert le < ltol and se < stol and np.isfinite(le + se + worst)
    assert not bad, ["%s: %.3e" % (k[-60:], rel_l2(got_of(k), G[k])) for k in bad]
    if V.VARIANTS[v]["ulm"]:
        assert float(np.abs(got_of(V.UE + "pad_doc")).max()) == 0.0


# ---------------------------------------------------------------------------------------------------------------- 1, 2: schedule A
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("v", V.NEW)
def test_schedule_a_every_step_equals_a_fresh_engine(v, dtype):
    """history_ref.SCHEDULE_A on one long-lived engine of the variant, every step (accumulation window) torch.equal to the same
    step on a fresh engine in losses, scores, S[:Rt] and the whole flat_g (the rule and the driver of
    tests/test_step_history_gpu.py): plain -> plan 128 -> plan 64 -> [encode_news, user_vectors] plan 128' -> plan 64' -> plain +
    hook -> plain -> SHORT (token feed; the oracle anchor) -> short plan 64 -> short -> full (token feed) -> [build_frozen_cache]
    plan 64 -> plain + hook -> window (plan 128, plan 64) -> plain + hook; fp16: scaler.mult 0.5, then 1.0.
    Under a hook every bucket fires, in order, and its slice of flat_g at that moment is what it holds after backward - bucket 0
    carries NRMS's W_Q / W_K / W_V gradients, which do not go through the recorded reduction tables.
    The eighth step (short batch, 1 700 rows) against O.model_fwd / O.model_bwd: _against_oracle."""
    t0 = time.perf_counter()
    eng = _loaded(v, dtype, HR.B_FULL)
    seen = {}

    def after(n, r, g, eng):
        seen[n] = g if r["anchor"] or r["only"] or n == 1 else None
        if r["anchor"]:
            assert n == 8 and r["feed"] == V.anchor_feed() and r["form"] == "tok"
            _against_oracle("anchor, step 8", v, dtype, r["feed"], g, eng)

    n = _play(dtype, HR.SCHEDULE_A, eng, after=after, model=v, snap=True)
    assert n == len(HR.SCHEDULE_A) - (2 if dtype == "bf16" else 0) and 8 in seen
    assert eng.fcache is not None and eng.B_alloc == HR.B_FULL and eng._clip_owner._acc_held == 0
    if dtype == "fp16":                                   # back at scale 1 on the first step's feed: the first step's bits
        assert eng.scaler.mult == 1.0 and all(torch.equal(seen[1][k], seen[n][k]) for k in WHAT)
    torch.cuda.synchronize()
    print("[variants %s %s] schedule A, %d steps, each against a fresh engine: %.2f s" % (v, dtype, n, time.perf_counter() - t0))


# ---------------------------------------------------------------------------------------------------------------- 3: a plan step
@pytest.mark.parametrize("v", V.NEW)
def test_a_plan_step_against_the_oracle(v):
    """p64_a under its plan (64 of 150 sequences encoded, resident feed, fp16) against the oracle, which sees the expanded token
    form: ties "a plan step equals a fresh plan step" to the reference for each pooling (tnr_pool_fwd / tnr_pool_bwd over the
    plan's n_enc sequences, tnr_segment_sum_rows in front of the encoder's backward)."""
    eng = _loaded(v, "fp16", HR.B_FULL)
    rec = HR.step("p64_a", plan=True)
    assert HR.n_enc(rec) == 64 < rec["B"] * (HR.U + HR.C)
    g = _run(eng, rec)
    torch.cuda.synchronize()
    assert eng.plan is not None and eng.plan.n_enc == 64
    _against_oracle("plan 64", v, "fp16", "p64_a", g, eng)


# ---------------------------------------------------------------------------------------------------------------- 4: feed forms
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("v", V.NEW)
def test_feed_forms_give_the_same_step(v, dtype):
    """As test_in_batch_dedup_gives_the_same_step and test_frozen_layer_cache_is_bit_identical (tests/test_engine_gpu.py) do for
    attention pooling: resident feed == token feed bit for bit; plan == no plan bit for bit in the forward, within 5e-3 (fp16) /
    3e-2 (bf16) relative L2 in the gradients (sum-then-backward against backward-then-sum in 16 bits), and bit for bit in the
    heads behind the expansion - the transform matrices and every student.user_encoder.* key, NRMS's W_* among them; through
    the frozen-layer cache both forms keep their bits."""
    eng = _loaded(v, dtype, HR.B_FULL)
    fid = "p64_a"
    plain, tok = _run(eng, HR.step(fid)), _run(eng, HR.step(fid, form="tok"))
    plan, plan_tok = _run(eng, HR.step(fid, plan=True)), _run(eng, HR.step(fid, plan=True, form="tok"))
    torch.cuda.synchronize()
    for k in WHAT:
        assert torch.equal(plain[k], tok[k]), "resident against token feed: %s" % k
        assert torch.equal(plan[k], plan_tok[k]), "resident against token feed under the plan: %s" % k
    for k in ("losses", "score", "S"):
        assert torch.equal(plain[k], plan[k]), "plan against no plan: %s" % k
    gtol, worst, behind = (5e-3 if dtype == "fp16" else 3e-2), 0.0, 0
    for k, (tr, o, cnt, _) in eng.slot.items():
        if not tr:
            continue
        a, b = plain["flat_g"][o:o + cnt], plan["flat_g"][o:o + cnt]
        if k.startswith(("transform_matrix.", V.UE)):
            assert torch.equal(a, b), "%s is behind the expansion and differs under the plan" % k
            behind += 1
            continue
        how = V.exempt(v, k)
        if how is not None:
            assert how == "noop" and float(b.abs().max()) < W.NOOP_ABS, k
            continue
        err = float((b - a).double().norm() / a.double().norm())
        worst = max(worst, err)
        assert err < gtol, "%s: %.3e" % (k, err)
    assert behind == 4 + 5 + (6 if V.VARIANTS[v]["nrms"] else 0) and all(k in eng.slot for k in (NRMS_KEYS if V.VARIANTS[v]["nrms"] else ()))
    print("\n[variants %s %s] plan against no plan: worst gradient relative L2 %.2e" % (v, dtype, worst))
    assert eng.build_frozen_cache(_shared(v)["comb"]) and eng.fcache is not None
    for want, rec in ((plain, HR.step(fid)), (plan, HR.step(fid, plan=True))):
        got = _run(eng, rec)
        torch.cuda.synchronize()
        for k in WHAT:
            assert torch.equal(got[k], want[k]), "through the frozen-layer cache (plan %s): %s" % (rec["plan"], k)


# ---------------------------------------------------------------------------------------------------------------- 5: optimiser layout
_OUT = {}


def _outside(eng, v):
    if v not in _OUT:
        _OUT[v] = torch.from_numpy(~V.slot_mask(eng.slot, eng.n_train)).to(DEV)
    return _OUT[v]


def _fill(eng, v, g, scale):
    """test_grad_clip_gpu.fill, then zeros outside the parameters' slots, as a backward leaves them: what lies between the slots
    then has zero gradient, moments and value, and no rate reaches it."""
    fill(eng, g, scale)
    eng.flat_g[_outside(eng, v)] = 0.0


def _everything(eng, v):
    n_in = int(V.slot_mask(eng.slot, eng.n_train).sum())
    return dict(ON, max_grad_norm=0.6 * GS * 1e-3 * float(np.sqrt(n_in)), ema_decay=DECAY)


@pytest.mark.parametrize("v", V.NEW)
def test_bucket_ranges_and_decay_map_tile_the_flat_buffer(v):
    """The assertions of test_bucket_ranges_and_decay_map_tile_the_flat_buffer_at_256 (tests/test_encoder_widths_gpu.py) on the
    variant's layout, with the mask derived from names: bucket_ranges() are contiguous and cover flat_g, no parameter straddles
    two buckets, decay_words has a bit for exactly the elements of the 2-D weights and none in a gap."""
    eng = _loaded(v, "fp16", 2)
    n = eng.n_train
    br = sorted(eng.bucket_ranges())
    assert br[0][0] == 0 and br[-1][1] == n == eng.flat_g.numel() and all(a[1] == b[0] for a, b in zip(br, br[1:]))
    mask = V.decay_table(eng.slot, n)
    words = E.decay_words(eng.slot, n)
    bits = np.unpackbits(words.view(np.uint8), bitorder="little").astype(bool)
    assert words.size == (n + 31) // 32 and np.array_equal(bits[:n], mask) and not bits[n:].any()
    covered = np.zeros(n, bool)
    for k, (tr, o, cnt, shp) in eng.slot.items():
        if tr:
            assert not covered[o:o + cnt].any() and cnt == int(np.prod(shp)), k
            covered[o:o + cnt] = True
            assert any(s <= o and o + cnt <= e for s, e in br), k
    assert np.array_equal(covered, V.slot_mask(eng.slot, n))
    assert mask.sum() == sum(cnt for k, (tr, o, cnt, shp) in eng.slot.items() if tr and A.decays(k, shp)) and not mask[~covered].any()
    assert np.array_equal(A.unpack(eng._decay_bits().cpu().numpy(), n), mask)
    first = min(o for k, (tr, o, cnt, shp) in eng.slot.items() if tr and ".bert_model." not in k)
    assert eng.bucket_ranges()[0] == (first, n)


@pytest.mark.parametrize("dtype,ams", [("fp16", True), ("bf16", False)])
@pytest.mark.parametrize("v", V.NEW)
def test_three_optimiser_steps_against_float64(v, dtype, ams):
    """Three Engine.step calls with three different rates (lr 2e-2, lr_bert 1e-2, lr_news_head 5e-3), weight decay 0.01, clipping
    (which clips steps 1 and 3), the schedule W = 2, T = 5 and ema_decay 0.9 against ema_ref.adamw_ema_step / adamw_ref.schedule /
    clip_ref.clip in float64, the per-element rates and the decay mask from parameter NAMES (variants_ref.rate_table).  Bounds of
    test_three_steps_against_float64 (tests/test_adamw_gpu.py, test_ema_gpu.py): p and the average rtol 1e-5 atol 1e-6; m, v, vmax
    rtol 1e-5 with a floor of 1e-5 of the buffer's largest magnitude.
    The same float64 run with lr_news_head replaced by lr_bert misses the engine's parameters - in the elements of
    student.news_encoder.dense.* (cls / mean) or attn.* + dense.* (att) and nowhere else: the middle range is where the names say."""
    eng = _loaded(v, dtype, 2)
    n = eng.n_train
    lr, mask = V.rate_table(eng.slot, n, RATES), V.decay_table(eng.slot, n)
    lr_alt = V.rate_table(eng.slot, n, (RATES[0], RATES[1], RATES[1]))
    head = V.head_elements(eng.slot, n)
    assert np.array_equal(lr != lr_alt, head) and head.any()
    kw = _everything(eng, v)
    ref, alt = ref_state(eng, ams), ref_state(eng, ams)
    p0 = ref[0].copy()
    e = e_alt = p0.copy()
    g = gen()
    for s, sc in enumerate((1e-3, 1e-4, 1e-3)):
        _fill(eng, v, g, sc)
        gh = eng.flat_g.cpu().numpy()
        eng.step(RATES[0], amsgrad=ams, **STEP, **kw)
        mult = A.schedule(s, WARM, TD)
        assert eng.lr_scale == mult == (0.0, 0.5, 1.0)[s]
        coef = C.clip([gh], kw["max_grad_norm"], GS)[1]
        assert (coef < 1.0) == (s != 1), (s, coef)                       # steps 1 and 3 are clipped, the small one is not
        *ref, e = M.adamw_ema_step(ref[0], gh, ref[1], ref[2], ref[3], e, s + 1, lr * mult, mask, WD, 1.0 - DECAY, grad_scale=GS * coef)
        *alt, e_alt = M.adamw_ema_step(alt[0], gh, alt[1], alt[2], alt[3], e_alt, s + 1, lr_alt * mult, mask, WD, 1.0 - DECAY,
                                       grad_scale=GS * coef)
        what = "variants %s %s ams%d step%d" % (v, dtype, ams, s + 1)
        compare(what, eng, ref, ams)
        compare_ema(what, eng, e)
        if s == 0:
            assert torch.equal(eng._ema, eng.flat[True])                   # rate 0: p kept its bits
    assert misses(eng, ref[0]) and misses(eng, p0) and eng.ema_updates == 3
    got = eng.flat[True].cpu().numpy().astype(np.float64)
    over = np.abs(got - alt[0]) > 1e-6 + 1e-5 * np.abs(alt[0])
    assert not over[~head].any() and over[head].mean() > 0.99, (int(over[~head].sum()), float(over[head].mean()))
    assert np.array_equal(A.unpack(eng._decay_map.cpu().numpy(), n), mask)
    if dtype == "fp16":
        eng.scaler.drain(eng)
        assert eng.scaler.skipped == 0 and eng.step_count == 3


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("v", V.NEW)
def test_bucketed_step_equals_the_whole_one(v, dtype):
    """As test_bucketed_equals_whole (tests/test_adamw_gpu.py, test_ema_gpu.py): a FakeSync over bucket_ranges() sends the update
    bucket by bucket, with decay, clipping, the schedule and the average on: bit for bit the step without sync."""
    outs = []
    for mode in ("whole", "bucketed"):
        eng = _loaded(v, dtype, 2)
        p0 = eng.flat[True].clone()
        g, ranges, kw = gen(), eng.bucket_ranges(), _everything(eng, v)
        for step in range(3):
            _fill(eng, v, g, 1e-3)
            sync = FakeSync(ranges) if mode == "bucketed" else None
            eng.step(RATES[0], amsgrad=dtype == "fp16", sync=sync, ema_warmup=True, **STEP, **kw)
            if sync is not None:
                assert sync.waited == list(range(len(ranges))) and not sync.pending
        outs.append(full_state(eng))
        if dtype == "fp16":
            eng.scaler.drain(eng)
            assert eng.scaler.skipped == 0
    assert len(outs[0]) == 6 and all(torch.equal(a, b) for a, b in zip(*outs))
    assert not torch.equal(outs[0][5], p0) and not torch.equal(outs[0][5], outs[0][0])


# ---------------------------------------------------------------------------------------------------------------- 6: checkpoint
@pytest.mark.parametrize("v,dtype", [("mean_ulm", "fp16"), ("cls_nrms", "bf16"), ("att_nrms_ulm", "fp16")])
def test_optimiser_checkpoint_split_equals_straight(v, dtype):
    """test_split_equals_straight's rule (tests/test_resume_gpu.py) on the variant's layout: three steps, optimizer_state_dict(), a
    fresh engine of the variant, load_state_dict + load_ema_state_dict + load_optimizer_state_dict, two more steps - torch.equal
    to five straight steps in parameters, moments, a 16-bit weight copy and the average; the saved state names exactly the
    variant's trainable keys."""
    from test_resume_gpu import drain, host, same, scaler_fields

    def run(eng, steps, kw):
        for s in steps:
            _fill(eng, v, torch.Generator(device=DEV).manual_seed(100 + s), 1e-3)
            eng.step(RATES[0], **STEP, **kw)

    straight = _loaded(v, dtype, 2)
    kw = _everything(straight, v)
    run(straight, range(3), kw)
    drain(straight)
    run(straight, range(3, 5), kw)
    first = _loaded(v, dtype, 2)
    run(first, range(3), kw)
    sd, esd, osd = host(first.state_dict()), host(first.ema_state_dict()), first.optimizer_state_dict()
    assert osd["step"] == 3 and osd["ema_updates"] == 3 and list(osd["state"]) == [k for k, s_ in first.slot.items() if s_[0]]
    assert set(osd["state"]) == set(V.oracle(v, V.anchor_feed())[2])
    del first
    second = _engine(dtype, 2, v)
    second.load_state_dict(sd)
    second.load_ema_state_dict(esd)
    second.load_optimizer_state_dict(osd)
    assert second.step_count == 3
    run(second, range(3, 5), kw)
    assert same(full_state(straight), full_state(second)) and len(full_state(second)) == 6
    drain(straight)
    drain(second)
    assert second.step_count == straight.step_count == 5 and scaler_fields(second) == scaler_fields(straight)
    assert second.ema_updates == straight.ema_updates == 5 and second.lr_scale == straight.lr_scale
    assert not torch.equal(second.flat[True], _loaded(v, dtype, 2).flat[True])


# ---------------------------------------------------------------------------------------------------------------- 7: overflow
def test_fp16_overflow_in_a_micro_batch_under_nrms_skips_the_whole_update():
    """cls_nrms, fp16, a window of two micro-batches at the short batch with an inf written into the accumulator as
    test_fp16_overflow_in_any_micro_batch_skips_the_whole_update_as_one (tests/test_grad_accum_gpu.py) does: parameters, moments
    and every 16-bit copy keep their bits and one step is counted as skipped; the next clean window and its step equal, bit for
    bit, those of an engine that never saw the overflow and runs at the same loss scale."""
    v = "cls_nrms"

    def window(eng, fids):
        for j, fid in enumerate(fids):
            _run(eng, HR.step(fid, micro=(j, len(fids))))

    def copies(eng):
        return [t.clone() for d in eng.sh for t in d.values()] + [eng.sh_a1.clone(), eng.sh_a1T.clone()]

    eng = _loaded(v, "fp16", HR.B_SHORT)
    _run(eng, HR.step("short_a", micro=(0, 2)))
    eng._acc[eng.off(NRMS_KEYS[0]) + 1] = float("inf")                   # as if micro-batch 0's backward had overflowed in W_Q's gradient
    _run(eng, HR.step("short_b", micro=(1, 2)))
    before, sh = state(eng)[:4], copies(eng)
    assert not bool(torch.isfinite(eng.flat_g).all()) and eng._acc_held == 0
    eng.step(1e-4, grad_scale=0.5)
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(before, state(eng)[:4]))
    assert all(torch.equal(a, b) for a, b in zip(sh, copies(eng)))
    eng.scaler.drain(eng)
    assert eng.scaler.skipped == 1 and eng.step_count == 0 and eng.scaler.mult == 0.5
    other = _loaded(v, "fp16", HR.B_SHORT)
    other.scaler.mult = eng.scaler.mult
    for e_ in (eng, other):
        window(e_, ("short_b", "short_a"))
        e_.step(1e-4, grad_scale=0.5)
        e_.scaler.drain(e_)
    assert torch.equal(eng.flat_g, other.flat_g) and bool(torch.isfinite(eng.flat_g).all())
    assert all(torch.equal(a, b) for a, b in zip(state(eng), state(other))) and all(torch.equal(a, b) for a, b in zip(copies(eng), copies(other)))
    assert (eng.scaler.skipped, eng.step_count, other.scaler.skipped, other.step_count) == (1, 1, 0, 1)
    assert not torch.equal(before[0], eng.flat[True])


# ---------------------------------------------------------------------------------------------------------------- 8: embeddings
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("v", V.EMBED)
def test_trainable_embeddings_against_autograd(v, dtype):
    """train_embeddings=True under mean and under cls pooling (additive user encoder), one step at the short batch in the token
    feed, against torch autograd in float32 (variants_ref.port_grads: oracle/torch_port.py with the pooling swapped, held to the
    numpy oracle by tests/test_variants_ref_cpu.py).  Bounds of test_trainable_embeddings_against_the_port
    (tests/test_encoder_widths_gpu.py): 1e-3 (fp16) / 1.6e-2 (bf16) of max(1, |ref|) on the total loss and the scores, 1.5e-2 /
    6e-2 relative L2 on every gradient; the word-table gradient exactly zero on every row the step does not name."""
    TOL, GTOL = {"bf16": 1.6e-2, "fp16": 1e-3}, {"bf16": 6e-2, "fp16": 1.5e-2}
    fid = V.anchor_feed()
    total_ref, score_ref, G = V.port_grads(v, fid)
    eng = _loaded(v, dtype, HR.B_SHORT, train_embeddings=True)
    assert set(EMB_KEYS) <= set(eng.grads) and eng.lo == 0
    rec = HR.step(fid, form="tok")
    g = _run(eng, rec)
    torch.cuda.synchronize()
    total = float(eng.total_loss().item())
    serr = np.abs(g["score"].cpu().numpy() - score_ref).max()
    worst = {}
    for k in eng.grads:
        how, got = V.exempt(v, k), eng.grad(k).cpu().numpy()
        if how == "zero":
            assert np.abs(got).max() == 0.0 and k not in G, k           # autograd leaves the unused pad_doc without a gradient
        elif how == "noop":
            assert np.abs(got).max() < W.NOOP_ABS, k
        else:
            worst[k] = rel_l2(got, G[k])
    assert {k for k in eng.grads if V.exempt(v, k) != "zero"} == set(G)
    wk = max(worst, key=worst.get)
    print("\n[variants embed %s %s] total %.6f autograd %.6f ; score max|err| %.2e ; embeddings %s ; worst %.2e (%s)" % (
        v, dtype, total, total_ref, serr, {k[len(E.BERT) + 11:]: "%.2e" % worst[k] for k in EMB_KEYS}, worst[wk], wk[-48:]))
    assert abs(total - total_ref) <= TOL[dtype] * max(1.0, abs(total_ref))
    assert serr <= TOL[dtype] * max(1.0, np.abs(score_ref).max())
    for k, err in worst.items():
        assert err < GTOL[dtype], "%s: relative L2 error %.3e" % (k, err)
    gw = eng.grad(WORD)
    named = _t(HR.named_tokens(rec))
    rest = torch.ones(gw.shape[0], dtype=torch.bool, device=DEV)
    rest[named] = False
    assert bool(rest[0]) and float(gw[rest].abs().max()) == 0.0 and float(gw[~rest].abs().max(1).values.min()) > 0.0
    assert np.array_equal(np.nonzero(np.abs(G[WORD]).max(1))[0], HR.named_tokens(rec))
