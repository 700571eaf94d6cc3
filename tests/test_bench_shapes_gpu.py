"""GPU parity of the dominant kernels AT THE LAUNCHES THE HEADLINE STEP ISSUES (B=32: M = 52 800 token rows).

Every (N, K, epilogue flags) engine.py passes to tnr_gemm_nt_ex / tnr_gemm_tn_wgrad in the 4-layer + 4-teacher step,
both 16-bit builds, multi-round grids (621 ... 2484 tiles on 256 CUs):
  * integer-valued asymmetric operands -> the main loop, the tile rasterisation (xcd_remap / tile_coords) and every tile
    variant are checked BIT-EXACT against numpy fp32 on rows sampled from every row tile (plus the ragged tail), and the
    full matrix against an fp32 GPU product that is itself pinned to numpy on those rows;
  * random operands -> the fused epilogues against numpy fp32 with the 16-bit output rounding as tolerance;
  * tnr_gemm_nt_route pins which kernel / tile height each launch takes (256-row, 224-row, 128x128 routes);
  * one B=32 forward (losses + scores) against the numpy oracle."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import tnr_hip as T                      # noqa: E402
from oracle import newsrec_oracle as O   # noqa: E402

DEV = "cuda:0"
M_BENCH = 52800                           # 32 impressions x 55 titles x 30 tokens
H, I, QPAD = 768, 3072, 256
TD = {"bf16": torch.bfloat16, "fp16": torch.float16}
EPS = {"bf16": 2.0 ** -8, "fp16": 2.0 ** -11}      # one rounding of the 16-bit output
TNPP_DEFAULT = 2                          # the library's default weight-gradient main loop (tnr_gemm_set_option "tnpp")
PIN_ROUTES = [True]                                # False while a test sizes the grids for another CU count than the device's

B_, G_, TH, R_, MD, F32O, AUX, CS = (T.EPI_BIAS, T.EPI_GELU, T.EPI_TANH, T.EPI_RES, T.EPI_MULDGELU, T.EPI_OUTF32, T.EPI_AUXOUT,
                                     T.EPI_COLSUM)
# (name, N, K, flags) of every NT launch of the headline step (engine.py: encode / backward_encoder)
NT_LAUNCHES = [
    ("qkv", 3 * H, H, B_),
    ("attn_out", H, H, B_ | R_),
    ("ffn_up_kept", I, H, B_ | G_ | AUX),
    ("ffn_up_frozen", I, H, B_ | G_),
    ("ffn_down", H, I, B_ | R_),
    ("pool_fc1", QPAD, H, B_ | TH | F32O),
    ("dgrad_pool", H, QPAD, R_),
    ("dgrad_w2_geluprime", I, H, MD | CS),
    ("dgrad_w1", H, I, R_),
    ("dgrad_o", H, H, 0),
    ("dgrad_qkv", H, 3 * H, R_),
]
WGRAD_LAUNCHES = [("qkv", 3 * H, H), ("attn_out", H, H), ("ffn_up", I, H), ("ffn_down", H, I), ("pool_fc1", QPAD, H)]


def _sfx(dtype):
    return "_f16" if dtype == "fp16" else ""


def _rows(M):
    """Rows sampled from every 224- and 256-row tile (stride 13 is coprime to both) + the ragged tail."""
    return np.unique(np.concatenate([np.arange(0, M, 13), np.arange(max(0, M - 300), M)]))


def _expected_route(M, N, flags, n_cu=256):
    if N % 256:
        return T.ROUTE_128 if (M <= 128 or flags & (G_ | MD)) else T.ROUTE_256x128
    t256, t224 = -(-M // 256) * (N // 256), -(-M // 224) * (N // 256)
    if M <= 128 or (t256 * 100 < n_cu * 60 and not flags & CS):
        return T.ROUTE_128
    c256, c224 = -(-t256 // n_cu) * 256, -(-t224 // n_cu) * 224
    return T.ROUTE_224 if (c224 * 108 < c256 * 100 and not flags & CS) else T.ROUTE_256


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("name,N,K,flags", NT_LAUNCHES)
def test_gemm_nt_main_loop_bit_exact_at_bench_shape(dtype, name, N, K, flags, route=None):
    M = M_BENCH
    rs = np.random.RandomState(N + K)
    A = rs.randint(-3, 4, (M, K)).astype(np.float32)
    Bm = rs.randint(-3, 4, (N, K)).astype(np.float32)
    Bm[:, 0] += np.arange(N) % 5                      # asymmetric: a row <-> col or tile swap cannot hide
    A[:, 1] += np.arange(M) % 3
    a, b = torch.from_numpy(A).to(DEV), torch.from_numpy(Bm).to(DEV)
    c = torch.full((M + 64, N), 7.0, device=DEV, dtype=torch.float32)
    got = T.query("tnr_gemm_nt_route" + _sfx(dtype), M, N, K, F32O)
    if route is not None:                            # a caller's explicit expectation (option "pp" = 0: no CU dependence)
        assert got == route, (name, got)
    elif PIN_ROUTES[0] and torch.cuda.get_device_properties(0).multi_processor_count == 256:
        assert got == _expected_route(M, N, F32O), (name, got)
    T.call("tnr_gemm_nt" + _sfx(dtype), a.to(TD[dtype]), K, b.to(TD[dtype]), K, c, N, M, N, K, None, None, 0, None, 0, F32O)
    full = a @ b.T                                    # fp32 GPU product: exact for these integers (|sum| < 2^24)
    torch.cuda.synchronize()
    rows = _rows(M)
    want = A[rows] @ Bm.T
    assert np.array_equal(full[rows].cpu().numpy(), want)            # pins the GPU checker to numpy
    assert np.array_equal(c[rows].cpu().numpy(), want), name         # the kernel against numpy
    assert torch.equal(c[:M], full), name                            # ... and every element of every tile
    assert (c[M:] == 7.0).all()                                      # nothing written past M


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("name,N,K,flags", NT_LAUNCHES)
def test_gemm_nt_epilogues_at_bench_shape(dtype, name, N, K, flags, route=None):
    M, td = M_BENCH, TD[dtype]
    g = torch.Generator(device=DEV).manual_seed(N * 7 + K + flags)
    rnd = lambda *s, sc=1.0: (torch.randn(*s, device=DEV, generator=g) * sc)
    a, b = rnd(M, K).to(td), rnd(N, K, sc=0.05).to(td)
    bias = rnd(N) if flags & B_ else None
    res = rnd(M, N).to(td) if flags & R_ else None
    aux = rnd(M, N).to(td) if flags & MD else (torch.zeros((M, N), device=DEV, dtype=td) if flags & AUX else None)
    aux_in = aux.clone() if flags & MD else None
    c = torch.zeros((M, N), device=DEV, dtype=torch.float32 if flags & F32O else td)
    # partial rows prefilled: every row of tnr_gemm_colsum_rows(M) is the kernel's, whatever the buffer held
    cs = torch.full((T.query("tnr_gemm_colsum_rows" + _sfx(dtype), M), N), 7.0, device=DEV) if flags & CS else None
    got = T.query("tnr_gemm_nt_route" + _sfx(dtype), M, N, K, flags)
    if route is not None:
        assert got == route, (name, got)
    elif PIN_ROUTES[0] and torch.cuda.get_device_properties(0).multi_processor_count == 256:
        assert got == _expected_route(M, N, flags), name
    T.call("tnr_gemm_nt_ex" + _sfx(dtype), a, K, b, K, c, N, M, N, K, bias, res, N if res is not None else 0, aux,
           N if aux is not None else 0, flags, cs)
    torch.cuda.synchronize()
    rows = _rows(M)
    ridx = torch.from_numpy(rows).to(DEV)
    f = lambda t: t[ridx].float().cpu().numpy()
    pre = f(a) @ b.float().cpu().numpy().T
    if bias is not None:
        pre = pre + bias.cpu().numpy()
    want = pre
    if flags & G_:
        want = O.gelu(pre)
    if flags & TH:
        want = np.tanh(pre)
    if flags & MD:
        want = pre * O.gelu_grad(f(aux_in))
    if flags & R_:
        want = want + f(res)
    eps = 1e-5 if flags & F32O else EPS[dtype]
    got = f(c)
    np.testing.assert_allclose(got, want, rtol=2 * eps, atol=2 * eps + 2e-5 * np.sqrt(K), err_msg=name)
    if flags & AUX:                                    # pre-activation stored beside the GELU output
        np.testing.assert_allclose(f(aux), pre, rtol=2 * eps, atol=2 * eps + 2e-5 * np.sqrt(K), err_msg=name + "/aux")
    if flags & CS:                                     # column sums of the ROUNDED 16-bit output (bias gradient)
        want_cs = c.float().sum(0).cpu().numpy()
        np.testing.assert_allclose(cs.sum(0).cpu().numpy(), want_cs, rtol=1e-4, atol=1e-2, err_msg=name + "/colsum")


# tnr_gemm_set_option "pp" = 0: the route of every NT launch with the epilogue flags (the main-loop check's fp32 output always takes
# the 256x128 kernel); the GELU / GELU' epilogues stay on the 128x128 kernel's table GELU
NT_ROUTES_WITHOUT_QUEUE = {"qkv": T.ROUTE_256x128, "attn_out": T.ROUTE_256x128, "ffn_up_kept": T.ROUTE_128,
                           "ffn_up_frozen": T.ROUTE_128, "ffn_down": T.ROUTE_256x128, "pool_fc1": T.ROUTE_256x128,
                           "dgrad_pool": T.ROUTE_256x128, "dgrad_w2_geluprime": T.ROUTE_128, "dgrad_w1": T.ROUTE_256x128,
                           "dgrad_o": T.ROUTE_256x128, "dgrad_qkv": T.ROUTE_256x128}


def test_gemm_nt_without_tile_queue_bit_exact():
    """tnr_gemm_set_option "pp" = 0 never launches the queue-fed persistent kernel (the way out when the (device, stream) table is
    full): every launch shape of the step then takes the 256x128 or 128x128 kernel, pinned, bit-exact and against numpy too."""
    L = T.lib()
    try:
        assert L.tnr_gemm_set_option(b"pp", 0) == 0
        for name, N, K, flags in NT_LAUNCHES:
            test_gemm_nt_main_loop_bit_exact_at_bench_shape("fp16", name, N, K, flags, route=T.ROUTE_256x128)
            test_gemm_nt_epilogues_at_bench_shape("fp16", name, N, K, flags, route=NT_ROUTES_WITHOUT_QUEUE[name])
        test_gemm_nt_epilogues_at_bench_shape("bf16", *NT_LAUNCHES[2], route=NT_ROUTES_WITHOUT_QUEUE[NT_LAUNCHES[2][0]])
    finally:
        L.tnr_gemm_set_option(b"pp", PP_DEFAULT)


PP_DEFAULT = 1                            # the library's default NT main loop (tnr_gemm_set_option "pp")


@pytest.mark.parametrize("cus", [128, 100, 8])
def test_gemm_grids_sized_for_fewer_cus_bit_exact(cus):
    """tnr_gemm_set_option "cus": the persistent kernels' grids and the NT panel plan sized for n CUs instead of the device's
    (two GEMMs side by side on disjoint shares, EXPERIMENTS.md section 4 item 20) - other panel heights, more tiles / units per
    workgroup, the same results on the step's launches."""
    L = T.lib()
    try:
        assert L.tnr_gemm_set_option(b"cus", cus) == 0
        PIN_ROUTES[0] = False
        for name, N, K, flags in NT_LAUNCHES if cus == 128 else NT_LAUNCHES[1:3]:
            test_gemm_nt_main_loop_bit_exact_at_bench_shape("fp16", name, N, K, flags)
            test_gemm_nt_epilogues_at_bench_shape("fp16", name, N, K, flags)
        for name, N, K in WGRAD_LAUNCHES if cus == 128 else WGRAD_LAUNCHES[:1]:
            test_gemm_tn_wgrad_bit_exact_at_bench_shape("fp16", name, N, K)
    finally:
        L.tnr_gemm_set_option(b"cus", 0)
        PIN_ROUTES[0] = True


def test_gemm_nt_routes_cover_every_tile_variant():
    """The three routes the engine's shapes can take, each pinned on a small integer-exact case as well."""
    if torch.cuda.get_device_properties(0).multi_processor_count != 256:
        pytest.skip("route table is written for 256 CUs")
    assert T.query("tnr_gemm_nt_route", M_BENCH, 768, 768, B_) == T.ROUTE_224
    assert T.query("tnr_gemm_nt_route", M_BENCH, 2304, 768, B_) == T.ROUTE_256
    assert T.query("tnr_gemm_nt_route", M_BENCH, 3072, 768, MD | CS) == T.ROUTE_256
    assert T.query("tnr_gemm_nt_route", 3300, 768, 768, B_) == T.ROUTE_128          # the B=2 goldens
    assert T.query("tnr_gemm_nt_route", M_BENCH, 384, 768, B_) == T.ROUTE_256x128   # N % 256 != 0


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("name,N,K", WGRAD_LAUNCHES)
def test_gemm_tn_wgrad_bit_exact_at_bench_shape(dtype, name, N, K):
    import engine as E
    M = M_BENCH
    Mp = (M + 127) // 128 * 128
    rs = np.random.RandomState(N + 3 * K)
    dY = np.zeros((Mp, N), np.float32)
    X = np.zeros((Mp, K), np.float32)
    dY[:M] = rs.randint(-2, 3, (M, N))
    X[:M] = rs.randint(-2, 3, (M, K))
    X[:M, 0] += np.arange(M) % 3
    dY[:M, 1] += np.arange(M) % 2
    splits = E.Engine._wgrad_splits(N, K)[0]                         # what the engine passes
    ws = torch.zeros(T.query("tnr_gemm_tn_ws_elems" + _sfx(dtype), N, K, splits), device=DEV)
    dW = torch.full((N, K), 3.0, device=DEV)
    dy, x = torch.from_numpy(dY).to(DEV).to(TD[dtype]), torch.from_numpy(X).to(DEV).to(TD[dtype])
    T.call("tnr_gemm_tn_wgrad" + _sfx(dtype), dy, N, x, K, dW, K, M, N, K, ws, splits, 0)
    torch.cuda.synchronize()
    want = dY.T @ X                                                  # |sum| <= 9 * 52800 < 2^24: exact in fp32
    assert np.array_equal(dW.cpu().numpy(), want), name
    T.call("tnr_gemm_tn_wgrad" + _sfx(dtype), dy, N, x, K, dW, K, M, N, K, ws, splits, 1)
    torch.cuda.synchronize()
    assert np.array_equal(dW.cpu().numpy(), 2 * want), name + "/accumulate"


def test_gemm_tn_wgrad_plain_loop_variant_bit_exact():
    """The weight gradient without the queue-fed persistent kernel (tnr_gemm_set_option "tnpp" = 0: the 256x128 kernel; the default
    is the persistent register-staged ping-pong loop) on the same launches."""
    L = T.lib()
    try:
        assert L.tnr_gemm_set_option(b"tnpp", 0) == 0
        for name, N, K in WGRAD_LAUNCHES:
            test_gemm_tn_wgrad_bit_exact_at_bench_shape("fp16", name, N, K)
    finally:
        L.tnr_gemm_set_option(b"tnpp", TNPP_DEFAULT)


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_gemm_tn_wgrad_register_staged_variant_bit_identical(dtype):
    """The weight gradient's two main loops (tnr_gemm_set_option "tnpp": 0 = the 256x128 kernel, operands by LDS-DMA + transposing
    fragment reads; 2 = the persistent ping-pong loop, operands through registers, transposed there, fragment-ready LDS image - the
    default) feed every MFMA the same operand registers in the same order: integer-exact on the step's launches, and the SAME BITS
    on random operands.  (tnpp = 0 ran a plain 256x256 loop before; it gave these bits too.)"""
    L = T.lib()
    M, Mp = M_BENCH, (M_BENCH + 127) // 128 * 128
    try:
        for tnpp in (0, 2):
            assert L.tnr_gemm_set_option(b"tnpp", tnpp) == 0
            for name, N, K in WGRAD_LAUNCHES:
                test_gemm_tn_wgrad_bit_exact_at_bench_shape(dtype, name, N, K)
        import engine as E
        g = torch.Generator(device=DEV); g.manual_seed(7)
        for name, N, K in WGRAD_LAUNCHES:
            dy = torch.zeros((Mp, N), device=DEV, dtype=TD[dtype]); x = torch.zeros((Mp, K), device=DEV, dtype=TD[dtype])
            dy[:M] = (torch.randn((M, N), device=DEV, generator=g) * 0.1).to(TD[dtype])
            x[:M] = torch.randn((M, K), device=DEV, generator=g).to(TD[dtype])
            splits = E.Engine._wgrad_splits(N, K)[0]
            ws = torch.zeros(T.query("tnr_gemm_tn_ws_elems" + _sfx(dtype), N, K, splits), device=DEV)
            outs = []
            for tnpp in (0, 2):
                L.tnr_gemm_set_option(b"tnpp", tnpp)
                dW = torch.zeros((N, K), device=DEV)
                T.call("tnr_gemm_tn_wgrad" + _sfx(dtype), dy, N, x, K, dW, K, M, N, K, ws, splits, 0)
                torch.cuda.synchronize()
                outs.append(dW)
            assert torch.equal(outs[0], outs[1]), name
            ref = dy[:M].float().T @ x[:M].float()
            assert (outs[1] - ref).abs().max().item() <= 2e-3 * ref.abs().max().item(), name
    finally:
        L.tnr_gemm_set_option(b"tnpp", TNPP_DEFAULT)


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_b32_forward_matches_oracle(dtype):
    """The benchmark's own forward (B=32, 4-layer student + 4 teachers, synthetic MIND-shaped inputs): the four losses and
    the (32, 5) scores against the numpy oracle on the same inputs, to the bound of the build."""
    import engine as E
    import hashinit
    import synth
    from schema import FULL, state_shapes
    nl, T_, B, n_news = 4, 4, 32, 4000
    cfg = E.EngineConfig(n_layers=nl, trainable_layers=(2, 3), num_teachers=T_)
    eng = E.Engine(cfg, DEV, max_batch=B, dtype=dtype)
    P = hashinit.init_state_dict(1234, state_shapes(FULL, nl, cfg.D, T_))
    eng.load_state_dict(P)
    comb = synth.news_table(1234, n_news, cfg.L)
    tabs = synth.teacher_tables(1234, T_, n_news, cfg.D)
    hidx, mask, cidx, label = synth.impressions(1235, B, n_news, cfg.U, cfg.C)
    d = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    losses, score = eng.forward_indexed(d(comb), d(hidx), d(mask), d(cidx), d(label), d(tabs))
    torch.cuda.synchronize()
    ocfg = dict(n_layers=nl, heads=12, trainable_layers=[2, 3], user_log_mask=False, temperature=1.0, coef=0.2)
    c64 = comb.astype(np.int64)
    ref = O.model_fwd(P, ocfg, c64[hidx], mask, c64[cidx], label, [tabs[i][hidx] for i in range(T_)],
                      [tabs[i][cidx] for i in range(T_)], keep=False)
    # losses (means over the batch): the north-star 1e-3 for fp16.  Logits: a MEASURED ALLOWANCE, not a target - the error budget
    # (tools/error_budget.py) puts the rounding of the WEIGHTS to the MFMA's 16-bit operand type alone at
    # max 2.1e-3 / r.m.s. 0.9e-3 over the 160 logits of this batch, every activation rounding together at 1.45e-3 / 0.5e-3, the
    # engine's total at 3.0e-3 / 1.02e-3; fp32 activation storage (any subset) would buy at most 0.5e-3 of it.  Bounded at 3e-3 max
    # (measured 2.6e-3) and 1.1e-3 r.m.s.
    tol_loss = {"fp16": 1e-3, "bf16": 1.6e-2}[dtype]
    tol_max, tol_rms = {"fp16": (3e-3, 1.1e-3), "bf16": (4e-2, 1.2e-2)}[dtype]
    l = losses.cpu().numpy()
    for got, key in ((l[0], "distill_loss"), (l[1], "target_loss"), (l[2], "emb_loss")):
        assert abs(got - float(ref[key])) <= tol_loss * max(1.0, abs(float(ref[key]))), (key, got, float(ref[key]))
    rs_ = ref["student_score"]
    err = np.abs(score.cpu().numpy() - rs_) / np.maximum(1.0, np.abs(rs_))
    rms = float(np.sqrt((err.astype(np.float64) ** 2).mean()))
    print("B=32 forward %s: score err / max(1,|ref|): max %.2e rms %.2e, |logit| max %.2f" % (dtype, err.max(), rms, np.abs(rs_).max()))
    import json
    print("PARITY_JSON " + json.dumps({"key": "b32", "dtype": dtype, "test": "tests/test_bench_shapes_gpu.py::test_b32_forward_matches_oracle",
                                       "what": "the benchmark's own forward at B = 32 against the fp32 oracle: logits / max(1, |ref|)",
                                       "logit_bound_max": tol_max, "logit_bound_rms": tol_rms, "logit_err_measured_max": float(err.max()),
                                       "logit_err_measured_rms": rms, "loss_bound_rel_to_max1_ref": tol_loss}))
    assert err.max() <= tol_max and rms <= tol_rms


def test_b32_training_is_bit_reproducible_run_to_run():
    """Two identical runs of the benchmark's step (B=32: multi-round grids of the queue-fed GEMM, one-round weight gradients,
    fixed-order reductions everywhere): every loss and the parameters after the updates agree bit for bit - the tile queue
    changes which workgroup computes a tile, never what it computes (tools/scratch/determinism_soak.py: the same over 400 steps)."""
    import engine as E
    import hashinit
    import synth
    from schema import FULL, state_shapes
    nl, T_, B, n_news, steps = 4, 4, 32, 4000, 4
    cfg = E.EngineConfig(n_layers=nl, trainable_layers=(2, 3), num_teachers=T_)
    d = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    comb, tabs = d(synth.news_table(1234, n_news, cfg.L)), d(synth.teacher_tables(1234, T_, n_news, cfg.D))
    hidx, mask, cidx, label = [d(x) for x in synth.impressions(1235, steps * B, n_news, cfg.U, cfg.C)]
    P = hashinit.init_state_dict(1234, state_shapes(FULL, nl, cfg.D, T_))

    def run():
        eng = E.Engine(cfg, DEV, max_batch=B, dtype="fp16")
        eng.load_state_dict(P)
        ls = []
        for i in range(steps):
            s = slice(i * B, (i + 1) * B)
            l, _ = eng.forward_indexed(comb, hidx[s], mask[s], cidx[s], label[s], tabs)
            ls.append(l.clone())
            eng.backward()
            eng.step(lr=1e-4)
        torch.cuda.synchronize()
        return torch.stack(ls).cpu(), eng.flat[True].cpu().clone(), eng.flat_g.cpu().clone()

    a, b = run(), run()
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_gemm_beside_held_cus_is_bit_identical():
    """The persistent NT kernel while another stream's kernel holds 24 CUs (tnr_debug_cu_hog: what the RCCL kernels of an
    overlapped all-reduce do): the workgroups that get no CU at launch start late and find the queue drained, the others take
    their tiles - same bits as the undisturbed launch, for a plain, a residual and a gelu' + column-sum launch; the
    weight-gradient kernel (a static one-round grid) as well."""
    from helpers import test_hooks
    hooks = test_hooks()
    M = M_BENCH
    td = torch.float16
    side = torch.cuda.Stream()
    rs = np.random.RandomState(3)
    for (N, K, flags) in ((3072, 768, 0), (768, 3072, T.EPI_BIAS | T.EPI_RES), (3072, 768, T.EPI_MULDGELU | T.EPI_COLSUM)):
        a = torch.from_numpy(rs.randn(M, K).astype(np.float32) * 0.5).to(DEV).to(td)
        b = torch.from_numpy(rs.randn(N, K).astype(np.float32) * 0.05).to(DEV).to(td)
        bias = torch.from_numpy(rs.randn(N).astype(np.float32)).to(DEV)
        res = torch.from_numpy(rs.randn(M, N).astype(np.float32) * 0.3).to(DEV).to(td) if flags & (T.EPI_RES | T.EPI_MULDGELU) else None
        csrows = T.query("tnr_gemm_colsum_rows_f16", M)
        outs = []
        for hog in (0, 24):
            c = torch.zeros((M, N), device=DEV, dtype=td)
            cs = torch.zeros((csrows, N), device=DEV) if flags & T.EPI_COLSUM else None
            torch.cuda.synchronize()
            if hog:
                with torch.cuda.stream(side):
                    assert hooks.tnr_debug_cu_hog(hog, 1500, side.cuda_stream) == 0
                torch.cuda._sleep(400000)                # let it take its CUs first
            for _ in range(3):                           # three launches inside the 1.5 ms: a late workgroup of one must not disturb the next
                T.call("tnr_gemm_nt_ex_f16", a, K, b, K, c, N, M, N, K, bias if flags & T.EPI_BIAS else None,
                       res if flags & T.EPI_RES else None, N if flags & T.EPI_RES else 0,
                       res if flags & T.EPI_MULDGELU else None, N if flags & T.EPI_MULDGELU else 0, flags, cs)
            torch.cuda.synchronize()
            outs.append((c, cs))
        assert torch.equal(outs[0][0], outs[1][0]), (N, K, flags)
        if outs[0][1] is not None:
            assert torch.equal(outs[0][1], outs[1][1])
    N, K = 3072, 768
    Mp = (M + 127) // 128 * 128
    dy = torch.zeros((Mp, N), device=DEV, dtype=td); dy[:M] = torch.from_numpy(rs.randn(M, N).astype(np.float32) * 0.1).to(DEV).to(td)
    x = torch.zeros((Mp, K), device=DEV, dtype=td); x[:M] = torch.from_numpy(rs.randn(M, K).astype(np.float32)).to(DEV).to(td)
    sp = 7
    ws = torch.zeros(int(T.query("tnr_gemm_tn_ws_elems", N, K, sp)), device=DEV)
    dws = []
    for hog in (0, 24):
        dw = torch.zeros((N, K), device=DEV)
        torch.cuda.synchronize()
        if hog:
            with torch.cuda.stream(side):
                assert hooks.tnr_debug_cu_hog(hog, 1500, side.cuda_stream) == 0
            torch.cuda._sleep(400000)
        T.call("tnr_gemm_tn_wgrad_f16", dy, N, x, K, dw, K, M, N, K, ws, sp, 0)
        torch.cuda.synchronize()
        dws.append(dw)
    assert torch.equal(dws[0], dws[1])


def test_queue_table_refuses_the_129th_stream_and_resets():
    """include/tnr_hip.h (tnr_gemm_queue_reset): the persistent GEMM keeps nine counters per (device, stream) in a 128-slot table;
    it never drains or switches a device - the 129th distinct stream is REFUSED (TNR_EUNSUPPORTED, message names the way out),
    bound streams keep working launch after launch, a reset leaves a stream usable, and option "pp" = 0 serves the refused one.
    Own process: the table stays full."""
    import json, os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "workers", "queue_table.py")], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    d = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert d["ok"] == 128 and d["refused_at"] == 128, d
    assert "(-2)" in d["msg"] and "pp" in d["msg"], d["msg"]
    assert d["again"] and d["rc_reset"] == 0 and d["after_reset"], d
    assert d["rc_unbound"] == -2 and d["plain_on_refused"], d
    # one table for the bf16 and the fp16 build, the NT and the weight-gradient kernel
    assert d["both_builds"] and d["refused_f16"] and d["rc_reset2"] == 0 and d["after_reset2"], d


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_wgrad_group_equals_separate_launches_bit_for_bit(dtype):
    """tnr_gemm_tn_wgrad_group: the four weight gradients of an encoder layer at the step's own size in ONE persistent launch
    (units of all four pulled from one queue) + one slab-sum launch == four tnr_gemm_tn_wgrad_ex calls, bit for bit (random
    operands; accumulate and out_scale mixed), and a group with a shape off the 256 x 256 route falls back to the same."""
    import engine as E
    M, td, sfx = M_BENCH, TD[dtype], _sfx(dtype)
    Mp = (M + 127) // 128 * 128
    g = torch.Generator(device=DEV).manual_seed(7)
    shapes = [(3 * H, H), (H, H), (I, H), (H, I)]
    probs, want = [], []
    for i, (N, K) in enumerate(shapes):
        dy = torch.zeros((Mp, N), device=DEV, dtype=td)
        x = torch.zeros((Mp, K), device=DEV, dtype=td)
        dy[:M] = (torch.randn((M, N), device=DEV, generator=g) * 0.1).to(td)
        x[:M] = torch.randn((M, K), device=DEV, generator=g).to(td)
        splits, elems = E.Engine._wgrad_splits(N, K)
        acc, scale = i & 1, (1.0, 1.0 / 1024, 0.5, 1.0)[i]
        base = torch.randn((N, K), device=DEV, generator=g)
        ref = base.clone()
        ws = torch.zeros(elems, device=DEV)
        T.call("tnr_gemm_tn_wgrad_ex" + sfx, dy, N, x, K, ref, K, M, N, K, ws, splits, acc, scale)
        want.append(ref)
        probs.append(dict(dY=dy, lddy=N, X=x, ldx=K, dW=base.clone(), lddw=K, M=M, N=N, K=K, ws=torch.zeros(elems, device=DEV),
                          splits=splits, accumulate=acc, out_scale=scale))
    T.wgrad_group(probs, f16=dtype == "fp16")
    torch.cuda.synchronize()
    for q, ref, (N, K) in zip(probs, want, shapes):
        assert torch.equal(q["dW"], ref), (N, K)
    # two of them a second time (a group of two, as under a gradient-bucket hook), and a group that cannot take the persistent route
    two = [dict(q, dW=torch.zeros_like(q["dW"]), accumulate=0) for q in probs[2:]]
    T.wgrad_group(two, f16=dtype == "fp16")
    N2, K2 = 384, 256
    dy2 = torch.zeros((Mp, N2), device=DEV, dtype=td)
    dy2[:M] = (torch.randn((M, N2), device=DEV, generator=g) * 0.1).to(td)
    sp2, el2 = E.Engine._wgrad_splits(N2, K2)
    odd = dict(dY=dy2, lddy=N2, X=probs[0]["X"], ldx=H, dW=torch.zeros((N2, K2), device=DEV), lddw=K2, M=M, N=N2, K=K2,
               ws=torch.zeros(el2, device=DEV), splits=sp2, accumulate=0, out_scale=1.0)
    ref2 = torch.zeros((N2, K2), device=DEV)
    T.call("tnr_gemm_tn_wgrad_ex" + sfx, dy2, N2, probs[0]["X"], H, ref2, K2, M, N2, K2, torch.zeros(el2, device=DEV), sp2, 0, 1.0)
    T.wgrad_group([odd, dict(probs[1], dW=torch.zeros_like(probs[1]["dW"]), accumulate=0)], f16=dtype == "fp16")
    torch.cuda.synchronize()
    assert torch.equal(odd["dW"], ref2)
    for q, (N, K) in zip(two, shapes[2:]):
        sp, el = E.Engine._wgrad_splits(N, K)
        ref = torch.zeros((N, K), device=DEV)
        T.call("tnr_gemm_tn_wgrad_ex" + sfx, q["dY"], N, q["X"], K, ref, K, M, N, K, torch.zeros(el, device=DEV), sp, 0, q["out_scale"])
        torch.cuda.synchronize()
        assert torch.equal(q["dW"], ref), (N, K)


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_wgrad_group_with_fewer_units_than_xcd_labels(dtype):
    """Two 256 x 256 gradients with one split each are two units: fewer than the eight XCD labels the grouped launch cuts its unit
    range over (a grid of two workgroups would leave the label that owns unit 1 without a workgroup and the slab sum would read an
    unwritten slab).  The entry point falls back to one launch per problem; results equal the single calls bit for bit."""
    td, sfx = TD[dtype], _sfx(dtype)
    g = torch.Generator(device=DEV).manual_seed(11)
    M, N, K = 700, 256, 256
    Mp = (M + 127) // 128 * 128
    probs, want = [], []
    for i in range(2):
        dy = torch.zeros((Mp, N), device=DEV, dtype=td); x = torch.zeros((Mp, K), device=DEV, dtype=td)
        dy[:M] = (torch.randn((M, N), device=DEV, generator=g) * 0.1).to(td)
        x[:M] = torch.randn((M, K), device=DEV, generator=g).to(td)
        ref = torch.zeros((N, K), device=DEV)
        T.call("tnr_gemm_tn_wgrad_ex" + sfx, dy, N, x, K, ref, K, M, N, K, torch.zeros(N * K, device=DEV), 1, 0, 1.0)
        want.append(ref)
        probs.append(dict(dY=dy, lddy=N, X=x, ldx=K, dW=torch.full((N, K), float("nan"), device=DEV), lddw=K, M=M, N=N, K=K,
                          ws=torch.full((N * K,), float("nan"), device=DEV), splits=1, accumulate=0, out_scale=1.0))
    T.wgrad_group(probs, f16=dtype == "fp16")
    torch.cuda.synchronize()
    for q, ref in zip(probs, want):
        assert torch.equal(q["dW"], ref)


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_wgrad_group_chained_problems_sum_two_row_ranges_of_one_gradient(dtype):
    """accumulate = 2 (stage 1: the title rows and the body rows of one Linear): the chained problem's slabs follow its
    predecessor's in the head's workspace and ONE slab sum covers both.  Checked against (a) the two single calls (write, then
    add): the same products, summed in another association, so equal to fp32 rounding; (b) an fp64 reference; (c) itself, run
    twice, bit for bit; (d) a chain off the persistent route (falls back to write + add: equal to (a) bit for bit); and a chain
    whose members disagree is refused."""
    td, sfx = TD[dtype], _sfx(dtype)
    g = torch.Generator(device=DEV).manual_seed(23)
    M1, M2 = 4800, 4096
    mk = lambda M, n: (torch.randn((M, n), device=DEV, generator=g) * 0.1).to(td)
    probs, want, ref64 = [], [], []
    for (N, K), (s1, s2), scale in (((3 * H, H), (4, 3), 1.0 / 1024), ((H, H), (14, 14), 1.0)):
        dy1, x1, dy2, x2 = mk(M1, N), mk(M1, K), mk(M2, N), mk(M2, K)
        ref = torch.full((N, K), float("nan"), device=DEV)
        ws = torch.zeros(16 * N * K, device=DEV)
        T.call("tnr_gemm_tn_wgrad_ex" + sfx, dy1, N, x1, K, ref, K, M1, N, K, ws, s1, 0, scale)
        T.call("tnr_gemm_tn_wgrad_ex" + sfx, dy2, N, x2, K, ref, K, M2, N, K, ws, s2, 1, scale)
        want.append(ref)
        ref64.append(((dy1.double().t() @ x1.double()) + (dy2.double().t() @ x2.double())) * scale)
        common = dict(dW=torch.full((N, K), float("nan"), device=DEV), lddw=K, N=N, K=K, out_scale=scale)
        probs.append(dict(common, dY=dy1, lddy=N, X=x1, ldx=K, M=M1, ws=torch.full(((s1 + s2) * N * K,), float("nan"), device=DEV),
                          splits=s1, accumulate=0))
        probs.append(dict(common, dY=dy2, lddy=N, X=x2, ldx=K, M=M2, ws=None, splits=s2, accumulate=2))
    T.wgrad_group(probs, f16=dtype == "fp16")
    torch.cuda.synchronize()
    first = [probs[0]["dW"].clone(), probs[2]["dW"].clone()]
    for got, ref, r64 in zip(first, want, ref64):
        scale_ = float(r64.abs().max())
        assert float((got - ref).abs().max()) <= 2e-6 * scale_                    # (a)
        assert float((got.double() - r64).abs().max()) <= 2e-5 * scale_           # (b): fp32 sums of ~9 000 16-bit products
    for q in probs:
        if q["accumulate"] == 0:
            q["dW"].fill_(float("nan"))
    T.wgrad_group(probs, f16=dtype == "fp16")
    torch.cuda.synchronize()
    assert torch.equal(probs[0]["dW"], first[0]) and torch.equal(probs[2]["dW"], first[1])     # (c)
    # (d) off the 256 x 256 route
    N, K = 384, 256
    dy1, x1, dy2, x2 = mk(M1, N), mk(M1, K), mk(M2, N), mk(M2, K)
    ref = torch.zeros((N, K), device=DEV)
    ws = torch.zeros(8 * N * K, device=DEV)
    T.call("tnr_gemm_tn_wgrad_ex" + sfx, dy1, N, x1, K, ref, K, M1, N, K, ws, 4, 0, 1.0)
    T.call("tnr_gemm_tn_wgrad_ex" + sfx, dy2, N, x2, K, ref, K, M2, N, K, ws, 4, 1, 1.0)
    common = dict(dW=torch.full((N, K), float("nan"), device=DEV), lddw=K, N=N, K=K, out_scale=1.0)
    odd = [dict(common, dY=dy1, lddy=N, X=x1, ldx=K, M=M1, ws=torch.zeros(8 * N * K, device=DEV), splits=4, accumulate=0),
           dict(common, dY=dy2, lddy=N, X=x2, ldx=K, M=M2, ws=None, splits=4, accumulate=2)]
    T.wgrad_group(odd, f16=dtype == "fp16")
    torch.cuda.synchronize()
    assert torch.equal(odd[0]["dW"], ref)
    with pytest.raises(T.TnrError):                            # a chain to another gradient
        T.wgrad_group([probs[0], dict(probs[3], accumulate=2)], f16=dtype == "fp16")
    with pytest.raises(T.TnrError):                            # a chain without a head
        T.wgrad_group([dict(probs[1]), probs[0]], f16=dtype == "fp16")
