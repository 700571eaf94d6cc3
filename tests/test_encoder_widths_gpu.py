"""GPU: whole training steps at every encoder width EngineConfig accepts - hidden in {256, 512, 768, 1024}, 64-wide heads, inter a
multiple of 256 or 128 x odd - against the CPU references (tests/widths_ref.py; pinned to each other by tests/test_widths_ref_cpu.py).

The kernel-level files sweep H, N, K and routes one kernel at a time; this file checks the code that composes them away from
768 / 12 / 3072: workspace sizes, the shadow-copy table, the weight-gradient splits off the 256 x 256 tiles, reduction strides of
3 H, dropout mask indices, the embedding backward's H / 256 variants, the K split of the small fp32 GEMMs, bucket ranges and the
fused optimiser step over another flat layout.  Tolerances are the ones the project already uses for the same comparison at 768
(named at each test); none is new."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import engine as E                                               # noqa: E402
import tnr_hip as T                                              # noqa: E402
import widths_ref as W                                           # noqa: E402
from embed_train_ref import EMB_KEYS, WORD, port_grads, rel_l2   # noqa: E402

DEV = "cuda:0"
ROUTES = {"128": (T.ROUTE_128,), "256x128": (T.ROUTE_256x128,), "pp": (T.ROUTE_256, T.ROUTE_224), "256": (T.ROUTE_256,)}


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _dev_inputs(inp):
    hist, mask, cand, label, th, tc = inp
    return _t(hist), _t(mask), _t(cand), _t(label), [_t(x) for x in th], [_t(x) for x in tc]


def _sfx(dtype):
    return "_f16" if dtype == "fp16" else ""


def _assert_routes(name, dtype, **kw):
    """The NT route of every GEMM the case issues (tnr_gemm_nt_route, on the 256 CUs the table was written for): a later routing
    change cannot quietly move a case off the path it is here for."""
    if torch.cuda.get_device_properties(0).multi_processor_count != 256:
        return
    c = W.WIDTH_CASES[name]
    M, want = W.rows(c), dict(c["routes"], **(c.get("routes_embed", {}) if kw.get("train_embeddings") else {}))
    for launch, N, K, flags in W.nt_launches(name, **kw):
        fl = sum(getattr(T, "EPI_" + f) for f in flags)
        got = T.query("tnr_gemm_nt_route" + _sfx(dtype), M, N, K, fl)
        assert got in ROUTES[want[launch]], "%s %s (M %d N %d K %d): route %d, expected %s" % (name, launch, M, N, K, got, want[launch])


# ---------------------------------------------------------------------------------------------------------------- a. stage-2 step
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("name", list(W.WIDTH_CASES))
def test_training_step_against_the_oracle(name, dtype):
    """Engine.forward + backward against O.model_fwd / O.model_bwd: the three losses, the student scores, every gradient of
    eng.grads.  Bounds of tools/fuzz_engine.py - fp16: loss 2e-3, score 3e-3 (of max(1, |ref|)), gradients 2e-2 relative L2;
    bf16: 1.6e-2, 2.4e-2, 8e-2.  No gradient is passed over: the no-op keys and an unused pad_doc are checked absolutely
    (widths_ref.exempt), every other one has an oracle norm >= 1e-7 (test_widths_ref_cpu.py)."""
    P, cfg, kw, inp = W.case(name)
    ref_l, ref_s, G = W.oracle(name)
    ltol, stol, gtol = W.TOLS[dtype]
    _assert_routes(name, dtype)
    eng = E.Engine(E.EngineConfig(**kw), DEV, max_batch=W.WIDTH_CASES[name]["B"], dtype=dtype)
    eng.load_state_dict(P)
    losses, score = eng.forward(*_dev_inputs(inp))
    eng.backward()
    torch.cuda.synchronize()
    le = np.abs(losses[:3].cpu().numpy() - ref_l).max() / max(1.0, np.abs(ref_l).max())
    se = np.abs(score.cpu().numpy() - ref_s).max() / max(1.0, np.abs(ref_s).max())
    assert set(eng.grads) == set(G)
    worst, wk, bad = W.compare_grads(name, list(eng.grads), lambda k: eng.grad(k).cpu().numpy(), G, gtol)
    print("\n[widths %s %s] %d rows: loss %.2e score %.2e worst gradient %.2e (%s)" % (name, dtype, W.rows(W.WIDTH_CASES[name]), le, se,
                                                                                     worst, wk[-48:]))
    assert le < ltol and se < stol
    assert not bad, ["%s: %.3e" % (k[-60:], rel_l2(eng.grad(k).cpu().numpy(), G[k])) for k in bad]
    assert np.isfinite(le + se + worst)


# ---------------------------------------------------------------------------------------------------------------- b. embeddings
_PORT = {}


def _port(name):
    """port_grads of a case with the embedding block trainable, computed once and shared (never modified)."""
    if name not in _PORT:
        P, cfg, _, inp = W.case(name)
        _PORT[name] = port_grads(P, cfg, *inp)
    return _PORT[name]


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("name", ["h256_i384_l19", "h1024_i2048_l24"])
def test_trainable_embeddings_against_the_port(name, dtype):
    """train_embeddings=True at hidden 256 and 1024: tnr_embed_ln_bwd's V = H / 256 = 1 and 4 inside a real backward (768 is V = 3)
    and the three tnr_colsum calls of _embed_bwd, against autograd of the torch port.  Bounds of tests/test_embed_train_gpu.py:
    1e-3 (fp16) / 1.6e-2 (bf16) of max(1, |ref|) on the loss and the scores, 1.5e-2 / 6e-2 relative L2 on gradients; word rows no
    token names exactly zero; the same bits under a bucket hook."""
    TOL, GTOL = {"bf16": 1.6e-2, "fp16": 1e-3}, {"bf16": 6e-2, "fp16": 1.5e-2}
    P, cfg, kw, inp = W.case(name)
    total_ref, score_ref, G = _port(name)
    _assert_routes(name, dtype, train_embeddings=True)
    eng = E.Engine(E.EngineConfig(train_embeddings=True, **kw), DEV, max_batch=W.WIDTH_CASES[name]["B"], dtype=dtype)
    assert set(EMB_KEYS) <= set(eng.grads)
    eng.load_state_dict(P)
    dev_in = _dev_inputs(inp)
    losses, score = eng.forward(*dev_in)
    eng.backward()
    torch.cuda.synchronize()
    total = float(eng.total_loss().item())
    serr = np.abs(score.cpu().numpy() - score_ref).max()
    worst = {}
    for k in eng.grads:
        how = W.exempt(name, k)
        got = eng.grad(k).cpu().numpy()
        if how == "zero":
            assert np.abs(got).max() == 0.0 and k not in G, k          # autograd leaves the unused pad_doc without a gradient
        elif how == "noop":
            assert np.abs(got).max() < W.NOOP_ABS, k
        else:
            worst[k] = rel_l2(got, G[k])
    assert {k for k in eng.grads if W.exempt(name, k) != "zero"} == set(G)
    wk = max(worst, key=worst.get)
    print("\n[widths embed %s %s] total %.6f port %.6f ; score max|err| %.2e ; embeddings %s ; worst %.2e (%s)" % (
        name, dtype, total, total_ref, serr, {k[len(E.BERT) + 11:]: "%.2e" % worst[k] for k in EMB_KEYS}, worst[wk], wk[-48:]))
    assert abs(total - total_ref) <= TOL[dtype] * max(1.0, abs(total_ref))
    assert serr <= TOL[dtype] * max(1.0, np.abs(score_ref).max())
    for k, err in worst.items():
        assert err < GTOL[dtype], "%s: relative L2 error %.3e" % (k, err)
    gw = eng.grad(WORD)
    named = torch.from_numpy(np.nonzero(np.abs(G[WORD]).max(1))[0]).to(DEV)
    rest = torch.ones(gw.shape[0], dtype=torch.bool, device=DEV)
    rest[named] = False
    assert rest[0] and float(gw[rest].abs().max()) == 0.0 and float(gw[named].abs().min(1).values.max()) > 0.0
    # under a bucket hook the reductions are flushed per bucket, the embedding block last: the same bits
    g_one = {k: eng.grad(k).clone() for k in eng.grads}
    eng.flat_g.zero_()
    fired = []
    eng.forward(*dev_in)
    eng.backward(after_bucket=fired.append)
    torch.cuda.synchronize()
    br = eng.bucket_ranges()
    assert fired == list(range(len(br))) and len(br) == 2 + 2 * len(kw["trainable_layers"]) and br[-1][0] == eng.off(WORD)
    assert all(torch.equal(g_one[k], eng.grad(k)) for k in g_one), [k for k in g_one if not torch.equal(g_one[k], eng.grad(k))]


# ---------------------------------------------------------------------------------------------------------------- c. stage 1, dropout
S1_SHAPES = {"h256_i384": dict(hidden=256, heads=4, inter=384),        # 128 x odd: the joint passes' shared-round weight gradients
             "h512_i1024": dict(hidden=512, heads=8, inter=1024)}      # cannot tile, the step runs per pass ; 256 x 4: joint
_S1 = {}


def _stage1_case(shape):
    """-> (P, cfg, inputs, seed, oracle output, oracle gradients) of a stage-1 step under dropout 0.1 / 0.1, computed once."""
    if shape not in _S1:
        import hashinit
        from helpers import FULL, state_shapes
        from oracle import dropout_oracle as DO
        from oracle import newsrec_oracle as O
        d = S1_SHAPES[shape]
        B, C, Lt, Lb, D, T_, nl, seed = 2, 2, 16, 64, 64, 2, 2, 4242
        dims = dict(FULL, H=d["hidden"], A=d["heads"], I=d["inter"], vocab=W.VOCAB, max_pos=W.MAX_POS)
        P = hashinit.init_state_dict(7, state_shapes(dims, nl, D, T_))
        cfg = dict(n_layers=nl, heads=d["heads"], trainable_layers=[0, 1])
        rs = np.random.RandomState(0)
        title = W._tokens(rs, B * C, Lt).reshape(B, C, 2 * Lt)
        body = W._tokens(rs, B, Lb)
        label = rs.randint(0, C, B)
        tt = [rs.randn(B, C, D).astype(np.float32) * 0.3 for _ in range(T_)]
        tb = [rs.randn(B, D).astype(np.float32) * 0.3 for _ in range(T_)]
        inp = (title, body, label, tt, tb)
        out = O.distill_fwd(P, cfg, *inp, drop_title=DO.Dropout(0.1, 0.1, seed, 0), drop_body=DO.Dropout(0.1, 0.1, seed, 1))
        _S1[shape] = (P, cfg, inp, seed, out, O.distill_bwd(P, cfg, out))
    return _S1[shape]


def _stage1_engine(shape, dtype):
    from stage1 import Stage1Engine
    P, cfg, inp, seed, _, _ = _stage1_case(shape)
    eng = Stage1Engine(n_layers=2, trainable_layers=(0, 1), num_teachers=2, npratio=1, title_len=16, body_len=64, device=DEV, batch=2,
                       dtype=dtype, news_dim=64, vocab=W.VOCAB, max_pos=W.MAX_POS, **S1_SHAPES[shape])
    eng.load_state_dict(P)
    eng.set_dropout(0.1, 0.1, seed)
    title, body, label, tt, tb = inp
    return eng, (_t(title), _t(body), _t(label), [_t(x) for x in tt], [_t(x) for x in tb])


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("shape", list(S1_SHAPES))
def test_stage1_step_with_dropout_against_the_oracle(shape, dtype):
    """Stage1Engine under set_dropout(0.1, 0.1, seed) against O.distill_fwd / O.distill_bwd under the same counter-based masks
    (dropout mask indices m * N + n with N = 256 / 384 / 512 / 1024 ...).  Bounds of tests/test_dropout_gpu.py: 1e-3 (fp16) / 1.6e-2
    (bf16) of max(1, |ref|) on losses, scores and news vectors, 1.5e-2 / 6e-2 relative L2 on gradients, no-op keys < 1e-3."""
    TOL, GTOL = {"bf16": 1.6e-2, "fp16": 1e-3}, {"bf16": 6e-2, "fp16": 1.5e-2}
    P, cfg, inp, seed, out, G = _stage1_case(shape)
    eng, d = _stage1_engine(shape, dtype)
    losses, score = eng.forward(*d)
    assert eng.ran_joint == (shape == "h512_i1024")
    torch.cuda.synchronize()
    tol, l = TOL[dtype], losses.cpu().numpy()
    got = dict(distill_loss=l[0], target_loss=l[1], emb_loss=l[2], total_loss=float(eng.total_loss().item()))
    sc = score.cpu().numpy()
    for k in got:
        assert abs(got[k] - float(out[k])) <= tol * max(1.0, abs(float(out[k]))), (k, got[k], float(out[k]))
    assert np.abs(sc - out["student_score"]).max() <= tol * max(1.0, np.abs(out["student_score"]).max())
    B, N = 2, 4
    S = eng.title.S.cpu().numpy()
    np.testing.assert_allclose(S[:N].reshape(out["title_vec"].shape), out["title_vec"], rtol=0, atol=tol * max(1.0, np.abs(out["title_vec"]).max()))
    np.testing.assert_allclose(S[N:N + B], out["body_vec"], rtol=0, atol=tol * max(1.0, np.abs(out["body_vec"]).max()))
    eng.backward()
    torch.cuda.synchronize()
    assert set(eng.title.grads) == set(G)
    worst, wk = 0.0, ""
    for k in eng.title.grads:
        ref, g = G[k], eng.grad(k).cpu().numpy()
        if k.endswith(W.NOOP):
            assert np.abs(g).max() < W.NOOP_ABS, k
            continue
        assert np.sqrt((ref.astype(np.float64) ** 2).sum()) >= W.MIN_NORM, k
        err = rel_l2(g, ref)
        if err > worst:
            worst, wk = err, k
        assert err < GTOL[dtype], "%s: relative L2 error %.3e" % (k, err)
    print("\n[widths stage1 %s %s] joint %d ; score max|err| %.2e ; worst gradient %.2e (%s)" % (
        shape, dtype, eng.ran_joint, np.abs(sc - out["student_score"]).max(), worst, wk[-48:]))


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_stage1_joint_passes_equal_the_per_pass_form_at_512(dtype):
    """As test_joint_passes_with_dropout_equal_the_per_pass_form: news vectors, scores and losses bit for bit, parameter gradients
    the same sums in another order (2e-5 relative L2)."""
    from test_stage1_joint_dropout_gpu import _compare, _step
    eng, d = _stage1_engine("h512_i1024", dtype)
    res = {}
    for joint in (False, True):
        eng.joint = joint
        res[joint] = _step(eng, lambda: eng.forward(*d))
        assert eng.ran_joint == joint
    worst = _compare(eng, res[True], res[False])
    eng.set_dropout(0.0, 0.0, 0)
    ev = _step(eng, lambda: eng.forward(*d))
    assert eng.ran_joint and not torch.equal(ev[2], res[True][2])          # the masks are live
    print("\n[widths stage1 joint 512 %s] worst relative L2 gap of a parameter gradient to the per-pass form: %.2e" % (dtype, worst))


# ---------------------------------------------------------------------------------------------------------------- d. inference
@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_inference_path_at_512(dtype):
    """encode_news + user_vectors at hidden 512 (the dense layer's K = 512: K split 2) against O.news_encoder_fwd and the oracle's user
    encoder, bounds of test_news_scoring_and_eval_user_vectors (1e-3 fp16 / 1.6e-2 bf16 of max(1, |ref|); user vectors rtol 1e-4,
    atol 1e-5 on the engine's own news vectors); and a news vector has the same bits alone and inside a larger pass - across row
    counts that route the QKV GEMM to the 128x128 kernel and to the persistent one
    (test_news_vectors_do_not_depend_on_the_batch_they_are_in)."""
    import hashinit
    from helpers import FULL, state_shapes
    from oracle import newsrec_oracle as O
    H, A, I, L, D, U, Q, n = 512, 8, 1152, 24, 128, 10, 72, 300
    P = hashinit.init_state_dict(7, state_shapes(dict(FULL, H=H, A=A, I=I, Q=Q, vocab=W.VOCAB, max_pos=W.MAX_POS), 2, D, 0))
    ec = E.EngineConfig(n_layers=2, trainable_layers=(), hidden=H, heads=A, inter=I, num_teachers=0, user_log_length=U, npratio=1,
                        num_words=L, news_dim=D, news_query=Q, user_query=Q, user_log_mask=True, vocab=W.VOCAB, max_pos=W.MAX_POS)
    eng = E.Engine(ec, DEV, max_batch=25, dtype=dtype)                    # 300 sequences, 7 200 token rows a pass
    eng.load_state_dict(P)
    comb = W._tokens(np.random.RandomState(11), n + 1, L).astype(np.int32)
    comb[0] = 0                                                            # the pad row of a resident table
    dcomb = _t(comb)
    ns = eng.encode_news(dcomb[:41])
    torch.cuda.synchronize()
    want, _ = O.news_encoder_fwd(P, comb[:41].astype(np.int64), 2, A)
    got = ns.cpu().numpy()
    assert got.shape == want.shape == (41, D)
    err = float((np.abs(got - want) / np.maximum(1.0, np.abs(want))).max())
    print("\n[widths inference 512 %s] news_scoring max |err| / max(1, |ref|) %.2e (|ref| max %.2f)" % (dtype, err, np.abs(want).max()))
    assert err <= {"fp16": 1e-3, "bf16": 1.6e-2}[dtype], err
    rs = np.random.RandomState(0)
    hidx = rs.randint(0, 41, (3, U)).astype(np.int32)
    mask = (rs.rand(3, U) > 0.5).astype(np.float32)
    mask[1] = 0
    uv = eng.user_vectors(ns, _t(hidx), _t(mask)).cpu().numpy()
    ref, _ = O.user_encoder_fwd(P, "student.user_encoder.", got[hidx], mask, True)
    np.testing.assert_allclose(uv, ref, rtol=1e-4, atol=1e-5)
    assert np.abs(uv[1]).max() == 0.0
    if torch.cuda.get_device_properties(0).multi_processor_count == 256:
        assert T.query("tnr_gemm_nt_route" + _sfx(dtype), 290 * L, 3 * H, H, T.EPI_BIAS) in ROUTES["pp"]
        assert T.query("tnr_gemm_nt_route" + _sfx(dtype), 33 * L, 3 * H, H, T.EPI_BIAS) == T.ROUTE_128
    ids = torch.arange(5, 295, dtype=torch.int32, device=DEV)
    whole = eng.encode(dcomb, 290, nidx=ids, train=False).clone()
    for m in (1, 7, 33, 110, 289):
        part = eng.encode(dcomb, m, nidx=ids[:m], train=False)
        assert torch.equal(part[:m], whole[:m]), m
    perm = torch.randperm(290, device=DEV)
    assert torch.equal(eng.encode(dcomb, 290, nidx=ids[perm], train=False)[:290], whole[perm])


# ---------------------------------------------------------------------------------------------------------------- e. optimiser
def _opt_engine(dtype):
    import hashinit
    from helpers import FULL, state_shapes
    cfg = E.EngineConfig(n_layers=2, trainable_layers=(0, 1), num_teachers=2, hidden=256, heads=4, inter=384, vocab=W.VOCAB,
                         max_pos=W.MAX_POS)
    if "P" not in _OPT:
        _OPT["P"] = hashinit.init_state_dict(3, state_shapes(dict(FULL, H=256, A=4, I=384, vocab=W.VOCAB, max_pos=W.MAX_POS), 2, cfg.D, 2))
    eng = E.Engine(cfg, DEV, max_batch=2, dtype=dtype)
    eng.load_state_dict(_OPT["P"])
    return eng


_OPT = {}


def test_bucket_ranges_and_decay_map_tile_the_flat_buffer_at_256():
    """bucket_ranges() are contiguous and cover flat_g; decay_words has a bit for exactly the elements of the 2-D weights
    (adamw_ref.decay_mask on the slot table), none in an alignment gap."""
    from test_adamw_gpu import tables
    eng = _opt_engine("fp16")
    br = sorted(eng.bucket_ranges())
    assert br[0][0] == 0 and br[-1][1] == eng.n_train == eng.flat_g.numel() and all(a[1] == b[0] for a, b in zip(br, br[1:]))
    _, mask = tables(eng)
    words = E.decay_words(eng.slot, eng.n_train)
    bits = np.unpackbits(words.view(np.uint8), bitorder="little").astype(bool)
    assert words.size == (eng.n_train + 31) // 32 and np.array_equal(bits[:eng.n_train], mask) and not bits[eng.n_train:].any()
    covered = np.zeros(eng.n_train, bool)
    for k, (tr, o, n, shp) in eng.slot.items():
        if tr:
            assert not covered[o:o + n].any() and n == int(np.prod(shp)), k
            covered[o:o + n] = True
            assert any(s <= o and o + n <= e for s, e in br), k          # no parameter straddles two buckets
    assert mask.sum() == sum(n for k, (tr, o, n, shp) in eng.slot.items() if tr and E.decays(k, shp)) and not mask[~covered].any()


@pytest.mark.parametrize("dtype,ams", [("fp16", True), ("bf16", False)])
def test_three_optimiser_steps_against_float64_at_256(dtype, ams):
    """Three Engine.step calls over the hidden 256 / inter 384 flat layout with weight decay 0.01, clipping (which clips the first
    step), the schedule W = 2, T = 5 and ema_decay 0.9, against tests/ema_ref.adamw_ema_step, adamw_ref.schedule and clip_ref.clip in
    float64.  Bounds of test_three_steps_against_float64 in tests/test_adamw_gpu.py / test_ema_gpu.py (their helpers are
    imported): p and the average rtol 1e-5 atol 1e-6; m, v, vmax rtol 1e-5 with a floor of 1e-5 of the buffer's largest magnitude."""
    import adamw_ref as A
    import clip_ref as C
    import ema_ref as M
    from test_adamw_gpu import GS, ON, RATES, TD, W as WARM, WD, compare, ref_state, tables
    from test_ema_gpu import DECAY, STEP, compare_ema, misses
    from test_grad_clip_gpu import fill, gen
    eng = _opt_engine(dtype)
    lr, mask = tables(eng)
    max_norm = 0.6 * GS * 1e-3 * float(np.sqrt(eng.n_train))
    ref = ref_state(eng, ams)
    p0 = ref[0].copy()
    e = p0.copy()
    g = gen()
    for s, sc in enumerate((1e-3, 1e-4, 1e-3)):
        fill(eng, g, sc)
        gh = eng.flat_g.cpu().numpy()
        eng.step(RATES[0], amsgrad=ams, ema_decay=DECAY, max_grad_norm=max_norm, **STEP, **ON)
        mult = A.schedule(s, WARM, TD)
        norm, coef = C.clip([gh], max_norm, GS)[:2]
        assert (coef < 1.0) == (s != 1), (s, coef)                       # steps 1 and 3 are clipped, the small one is not
        *ref, e = M.adamw_ema_step(ref[0], gh, ref[1], ref[2], ref[3], e, s + 1, lr * mult, mask, WD, 1.0 - DECAY, grad_scale=GS * coef)
        what = "widths 256/384 %s ams%d step%d" % (dtype, ams, s + 1)
        compare(what, eng, ref, ams)
        compare_ema(what, eng, e)
        if s == 0:
            assert torch.equal(eng._ema, eng.flat[True])                   # rate 0: p kept its bits
    assert misses(eng, ref[0]) and misses(eng, p0)
    assert eng.ema_updates == 3
    if dtype == "fp16":
        eng.scaler.drain(eng)
        assert eng.scaler.skipped == 0 and eng.step_count == 3


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_bucketed_step_equals_the_whole_one_at_256(dtype):
    """As test_bucketed_equals_whole (tests/test_adamw_gpu.py, test_ema_gpu.py): the bucket-by-bucket update with decay, clipping,
    the schedule and the average on, bit for bit the step without sync - over bucket x range boundaries of the 256 / 384 layout."""
    from test_adamw_gpu import GS, ON, RATES
    from test_ema_gpu import DECAY, STEP, full_state
    from test_grad_clip_gpu import FakeSync, fill, gen
    outs = []
    for mode in ("whole", "bucketed"):
        eng = _opt_engine(dtype)
        p0 = eng.flat[True].clone()
        g = gen()
        ranges = eng.bucket_ranges()
        for step in range(3):
            fill(eng, g, 1e-3)
            sync = FakeSync(ranges) if mode == "bucketed" else None
            eng.step(RATES[0], amsgrad=dtype == "fp16", sync=sync, ema_decay=DECAY, ema_warmup=True,
                     max_grad_norm=0.6 * GS * 1e-3 * float(np.sqrt(eng.n_train)), **STEP, **ON)
            if sync is not None:
                assert sync.waited == list(range(len(ranges))) and not sync.pending
        outs.append(full_state(eng))
        if dtype == "fp16":
            eng.scaler.drain(eng)
            assert eng.scaler.skipped == 0
    assert len(outs[0]) == 6 and all(torch.equal(a, b) for a, b in zip(*outs))
    assert not torch.equal(outs[0][5], p0) and not torch.equal(outs[0][5], outs[0][0])


# ---------------------------------------------------------------------------------------------------------------- f. drop-in surface
def test_model_from_a_512_wide_config_and_checkpoint(tmp_path):
    """model_bert.Model(args) with a config.json of hidden 512, 8 heads, inter 1152 and a unilm2-layout checkpoint of that shape
    (test_construction_time_init_and_pretrained_import at 768): the import fills the encoder, and engine.encode matches
    O.news_encoder_fwd on the imported weights within that test's bound, 3e-2 of max |ref| + 1e-5."""
    import json
    import types
    import model_bert
    from helpers import unilm_checkpoint
    from oracle import newsrec_oracle as O
    from tnlrv3 import convert_state_dict as C
    H, A, I, vocab, L, D = 512, 8, 1152, 600, 30, 64
    cfgp = tmp_path / "config.json"
    cfgp.write_text(json.dumps(dict(hidden_size=H, num_attention_heads=A, intermediate_size=I, vocab_size=vocab,
                                    max_position_embeddings=48, type_vocab_size=2, layer_norm_eps=1e-12)))
    raw = unilm_checkpoint(5, H, 3, A, I, vocab, 32)          # 3 layers and 32 positions in the checkpoint
    ck = tmp_path / "unilm2-small.bin"
    torch.save(raw, ck)
    args = types.SimpleNamespace(
        config_name=str(cfgp), model_name=str(ck), pooling="att", model="NAML", num_teacher_layers=12, num_student_layers=2,
        bert_trainable_layer=[1], news_dim=D, news_query_vector_dim=200, user_query_vector_dim=200, num_teachers=1,
        user_log_length=4, npratio=1, num_words_title=L, user_log_mask=False, temperature=1.0, coef=0.2, batch_size=2)
    torch.cuda.set_device(0)
    model = model_bert.Model(args)
    ec = model.engine.cfg
    assert (ec.H, ec.A, ec.I, ec.vocab, ec.max_pos) == (H, A, I, vocab, 48)
    missing, unexpected = model.pretrained_report
    assert sorted(missing) == ["student.news_encoder.bert_model.classifier.bias", "student.news_encoder.bert_model.classifier.weight"]
    assert "cls.predictions.bias" in unexpected and any(k.startswith("bert.encoder.layer.2.") for k in unexpected)
    sd = {k: v.cpu().numpy() for k, v in model.state_dict().items()}
    pfx = "student.news_encoder.bert_model."
    conv = C.load_model(dict(raw))
    for k in ("bert.encoder.layer.1.attention.self.key.weight", "bert.encoder.layer.0.attention.self.value.bias",
              "bert.encoder.layer.1.intermediate.dense.weight", "bert.encoder.layer.0.output.dense.weight",
              "bert.rel_pos_bias.weight", "bert.embeddings.word_embeddings.weight", "bert.pooler.dense.weight"):
        assert np.array_equal(sd[pfx + k], conv[k].numpy()), k
    assert sd[pfx + "bert.encoder.layer.1.intermediate.dense.weight"].shape == (I, H) and sd[pfx + "bert.rel_pos_bias.weight"].shape == (A, 32)
    assert not sd[pfx + "bert.encoder.layer.0.attention.self.key.bias"].any()
    pos = sd[pfx + "bert.embeddings.position_embeddings.weight"]
    assert pos.shape == (48, H) and np.array_equal(pos[:32], raw["bert.embeddings.position_embeddings.weight"].numpy())
    assert 0.015 < pos[32:].std() < 0.025                                  # new rows ~ N(0, 0.02)
    w = sd["student.news_encoder.dense.weight"]
    assert abs(w).max() <= 1 / np.sqrt(H) + 1e-6 and w.std() > 0.5 / np.sqrt(3 * H)
    ids = np.zeros((6, 2 * L), dtype=np.int64)
    rng = np.random.RandomState(0)
    for r in range(6):
        n = 5 + 4 * r
        ids[r, :n] = rng.randint(1, vocab, n)
        ids[r, L:L + n] = 1
    got = model.engine.encode(torch.from_numpy(ids).cuda(), 6).cpu().numpy()
    ref, _ = O.news_encoder_fwd(sd, ids, 2, A, None)
    print("\n[widths drop-in 512] imported-encoder max|err| %.3e (|ref| max %.3e)" % (np.abs(got - ref).max(), np.abs(ref).max()))
    assert np.abs(got - ref).max() <= 3e-2 * np.abs(ref).max() + 1e-5
