"""CPU side of global-norm gradient clipping (--max_grad_norm): tests/clip_ref.py is torch.nn.utils.clip_grad_norm_, the flag
defaults to off beside the unchanged reference flags, the partial-count query answers without a GPU, and an engine that was never
asked to clip holds no clipping buffer."""
import json
import os

import numpy as np
import torch

import clip_ref as C
import tnr_hip as T
from conftest import GOLDEN

IFACE = json.load(open(os.path.join(GOLDEN, "interface.json")))


def test_clip_ref_is_torch_clip_grad_norm():
    """Norm and scaled gradients of the float64 formula == clip_grad_norm_ on float64 CPU tensors split into several parameters,
    for a threshold below the norm (clips) and one above it (coefficient exactly 1)."""
    rs = np.random.RandomState(3)
    shapes = [(7, 5), (33,), (2, 3, 4), (1,)]
    grads = [rs.standard_normal(s) * 10.0 ** rs.randint(-3, 1) for s in shapes]
    true = float(np.sqrt(sum((g ** 2).sum() for g in grads)))
    for max_norm in (0.5 * true, 2.0 * true):
        ps = [torch.zeros(s, dtype=torch.float64, requires_grad=True) for s in shapes]
        for p, g in zip(ps, grads):
            p.grad = torch.from_numpy(g.copy())
        got = float(torch.nn.utils.clip_grad_norm_(ps, max_norm, norm_type=2))
        total, coef = C.clip(grads, max_norm)
        assert abs(got - total) <= 1e-14 * total and abs(total - true) <= 1e-14 * true
        assert (coef == 1.0) == (max_norm > true)
        for p, g in zip(ps, grads):
            np.testing.assert_allclose(p.grad.numpy(), coef * g, rtol=1e-14, atol=0.0)
    # grad_scale: the norm is that of the scaled gradient
    total, coef = C.clip(grads, 0.25 * true, grad_scale=0.5)
    assert abs(total - 0.5 * true) <= 1e-14 * true and abs(coef - 0.25 * true / (0.5 * true + 1e-6)) <= 1e-14
    # fp32 overflow of the sum of squares is the kernels' business; the float64 formula itself: inf -> 0, nan -> nan
    assert C.clip([np.array([np.inf, 1.0])], 1.0) == (np.inf, 0.0)
    assert np.isnan(C.clip([np.array([np.nan, 1.0])], 1.0)[1])


def test_flag_defaults_to_off_and_reference_flags_keep_their_defaults():
    import parameters
    a = vars(parameters.parse_args([]))
    assert a["max_grad_norm"] == 0.0 and isinstance(a["max_grad_norm"], float)
    for k, v in IFACE["flags"].items():
        assert a[k] == v, "--%s default %r != reference %r" % (k, a[k], v)
    assert "max_grad_norm" not in IFACE["flags"]
    assert parameters.parse_args(["--max_grad_norm", "0.5"]).max_grad_norm == 0.5
    import post_train_kd
    assert post_train_kd.parse_args([]).max_grad_norm == 0.0
    assert post_train_kd.parse_args(["--max_grad_norm", "2"]).max_grad_norm == 2.0


def test_sumsq_parts_without_a_gpu():
    """tnr_grad_sumsq_parts: host-only; >= 1, non-decreasing in n, bounded, and what tests/clip_ref.py restates."""
    ns = [1, 3, 4, 4095, 4096, 4097, 3 * 4096 + 5, 4096 * 2047, 4096 * 2048, 4096 * 2048 + 1, 38_600_000, 1 << 33]
    got = [T.query("tnr_grad_sumsq_parts", n) for n in ns]
    assert got == [C.sumsq_parts(n) for n in ns]
    assert got[0] == 1 and all(a <= b for a, b in zip(got, got[1:])) and got[-1] == C.GRID_CAP
    assert [T.query("tnr_grad_sumsq_parts", n) for n in (4096, 4097)] == [1, 2]
    assert C.sumsq_depth(4096) == 15 and C.sumsq_depth(C.BLOCK * C.GRID_CAP + 1) == 19


def test_engine_without_clipping_allocates_nothing_new():
    import engine as E
    eng = E.Engine(E.EngineConfig(n_layers=1, trainable_layers=(0,), num_teachers=1), device="cpu", max_batch=1)
    assert eng._clip_state is None and eng._clip_owner is eng and eng.grad_norm() is None
    second = E.Engine(eng.cfg, device="cpu", max_batch=1, share=eng)
    assert second._clip_owner is eng and second._clip_state is None and second.grad_norm() is None
    assert not [k for k, v in vars(eng).items() if "clip" in k and isinstance(v, torch.Tensor)]
