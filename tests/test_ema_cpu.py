"""CPU side of the exponential moving average of the weights (--ema_decay, --ema_warmup, --use_ema): tests/ema_ref.py is
torch.optim.swa_utils.AveragedModel with get_ema_multi_avg_fn on top of torch.optim.AdamW, engine.ema_decay_at is ema_ref.decay_at,
the flags default to off beside the unchanged reference flags, and TnrAdam hands the arguments to the engine only when on."""
import json
import os

import numpy as np
import pytest
import torch

import ema_ref as M
from conftest import GOLDEN

IFACE = json.load(open(os.path.join(GOLDEN, "interface.json")))


@pytest.mark.parametrize("ams", [True, False])
def test_ema_ref_is_torch_averaged_model(ams):
    """Twelve float64 steps of torch.optim.AdamW on a small module, the average kept by AveragedModel(multi_avg_fn =
    get_ema_multi_avg_fn(0.9)) and seeded from the parameters before training.  AveragedModel COPIES on its first
    update_parameters call (n_averaged == 0), so that call is made before the first step - the copy is the seed - and every later
    call, one behind each optimiser step, is an average.  Bound 1e-12 on the parameters and on the average."""
    from torch.optim.swa_utils import AveragedModel, get_ema_multi_avg_fn
    decay, wd, lr, steps = 0.9, 0.1, 1e-2, 12
    torch.manual_seed(3)
    model = torch.nn.Sequential(torch.nn.Linear(5, 4), torch.nn.Tanh(), torch.nn.Linear(4, 3)).double()
    params = list(model.parameters())
    opt = torch.optim.AdamW(params, lr=lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=wd, amsgrad=ams)
    avg = AveragedModel(model, multi_avg_fn=get_ema_multi_avg_fn(decay))
    avg.update_parameters(model)                                   # the first call copies: the seed
    assert int(avg.n_averaged) == 1
    # per parameter: p, m, v, vmax, ema - the average starts as the parameters before training
    ref = [[p.detach().numpy().copy(), np.zeros(p.shape), np.zeros(p.shape), np.zeros(p.shape) if ams else None,
            p.detach().numpy().copy()] for p in params]
    p0 = [r[0].copy() for r in ref]
    x = torch.randn(steps, 7, 5, dtype=torch.float64)
    for s in range(steps):
        opt.zero_grad()
        model(x[s]).square().sum().backward()
        grads = [p.grad.detach().numpy().copy() for p in params]
        opt.step()
        avg.update_parameters(model)
        for i, (p, a) in enumerate(zip(params, avg.module.parameters())):
            q, m, v, vm, e = ref[i]
            ref[i] = list(M.adamw_ema_step(q, grads[i], m, v, vm, e, s + 1, lr, True, wd, 1.0 - decay))
            err_p = float(np.abs(p.detach().numpy() - ref[i][0]).max())
            err_e = float(np.abs(a.detach().numpy() - ref[i][4]).max())
            print("[ema] ams%d step %d param %d: max|err| p %.3e, ema %.3e, err / bound %.4f" % (
                ams, s + 1, i, err_p, err_e, max(err_p, err_e) / 1e-12))
            assert err_p <= 1e-12 and err_e <= 1e-12
    assert int(avg.n_averaged) == steps + 1
    # the average is neither the trained parameters nor the seed
    assert all(np.abs(r[4] - r[0]).max() > 1e-4 and np.abs(r[4] - q).max() > 1e-4 for r, q in zip(ref, p0))
    # a skipped step leaves all five untouched
    q, m, v, vm, e = ref[0]
    out = M.adamw_ema_step(q, np.full(q.shape, np.inf), m, v, vm, e, steps + 1, lr, True, wd, 1.0 - decay, skipped=True)
    assert all(a is b or np.array_equal(a, b) for a, b in zip(out, ref[0]))


def test_ema_step_values():
    e, p = np.array([1.0, -2.0, 0.5]), np.array([3.0, 2.0, 0.5])
    assert np.array_equal(M.ema_step(e, p, 1.0), p) and np.array_equal(M.ema_step(e, p, 0.0), e)
    assert np.allclose(M.ema_step(e, p, 0.25), 0.75 * e + 0.25 * p, rtol=1e-15, atol=0.0)


def test_engine_decay_rule_is_the_reference_rule():
    """engine.ema_decay_at == ema_ref.decay_at for u = 0 .. 40, warm-up on and off; the warm-up is TF's (1 + u) / (10 + u), capped."""
    import engine as E
    for decay in (0.9, 0.999, 0.5):
        for warm in (False, True):
            assert [E.ema_decay_at(u, decay, warm) for u in range(41)] == [M.decay_at(u, decay, warm) for u in range(41)]
    assert [M.decay_at(u, 0.9, False) for u in (0, 7, 40)] == [0.9, 0.9, 0.9]
    assert M.decay_at(0, 0.999, True) == 0.1 and M.decay_at(1, 0.999, True) == 2.0 / 11.0 and M.decay_at(8, 0.999, True) == 0.5
    assert M.decay_at(80, 0.9, True) == 0.9 and M.decay_at(81, 0.9, True) == 0.9 and M.decay_at(79, 0.9, True) == 80.0 / 89.0
    assert E.ema_decay_at(3, 0.9) == 0.9                                   # warm-up defaults to off


def test_flags_default_to_off_and_reference_flags_keep_their_defaults():
    import parameters
    import post_train_kd
    a = vars(parameters.parse_args([]))
    assert a["ema_decay"] == 0.0 and isinstance(a["ema_decay"], float)
    assert a["ema_warmup"] is False and a["use_ema"] is False
    for k, v in IFACE["flags"].items():
        assert a[k] == v, "--%s default %r != reference %r" % (k, a[k], v)
    assert not {"ema_decay", "ema_warmup", "use_ema"} & set(IFACE["flags"])
    b = parameters.parse_args(["--ema_decay", "0.999", "--ema_warmup", "True", "--mode", "test", "--use_ema", "True"])
    assert (b.ema_decay, b.ema_warmup, b.use_ema, b.mode) == (0.999, True, True, "test")
    c = post_train_kd.parse_args([])
    assert (c.ema_decay, c.ema_warmup) == (0.0, False)
    d = post_train_kd.parse_args(["--ema_decay", "0.99", "--ema_warmup", "True"])
    assert (d.ema_decay, d.ema_warmup) == (0.99, True)
    from model_bert import TnrAdam
    o = TnrAdam(None, 1e-4)
    assert (o.ema_decay, o.ema_warmup) == (0.0, False)


class _StubEngine:
    def __init__(self):
        self.calls = []

    def step(self, lr, **kw):
        self.calls.append((lr, kw))


class _StubModel:
    def __init__(self):
        self.engine = _StubEngine()


def test_tnr_adam_forwards_the_average_only_when_on():
    from model_bert import TnrAdam
    base = {"grad_scale", "lr_bert", "lr_news_head", "sync"}
    for kw in ({}, dict(ema_decay=0.0), dict(ema_decay=None), dict(ema_decay=0.0, ema_warmup=True)):
        m = _StubModel()
        TnrAdam(m, 1e-4, **kw).step()
        (lr, got), = m.engine.calls
        assert lr == 1e-4 and set(got) == base, got
    m = _StubModel()
    TnrAdam(m, 1e-4, ema_decay=0.99).step()
    assert m.engine.calls[0][1]["ema_decay"] == 0.99 and m.engine.calls[0][1]["ema_warmup"] is False
    assert set(m.engine.calls[0][1]) == base | {"ema_decay", "ema_warmup"}
    m = _StubModel()
    TnrAdam(m, 1e-4, ema_decay=0.9, ema_warmup=True, weight_decay=0.01).step()
    got = m.engine.calls[0][1]
    assert got["ema_decay"] == 0.9 and got["ema_warmup"] is True and got["weight_decay"] == 0.01
    assert set(got) == base | {"ema_decay", "ema_warmup", "weight_decay", "warmup_steps", "lr_decay_steps"}


def test_engine_without_the_average_allocates_nothing_new():
    import engine as E
    eng = E.Engine(E.EngineConfig(n_layers=1, trainable_layers=(0,), num_teachers=1), device="cpu", max_batch=1)
    assert eng._ema is None and eng.ema_state_dict() is None and eng.ema_updates == 0
    second = E.Engine(eng.cfg, device="cpu", max_batch=1, share=eng)
    assert second._ema is None and second.ema_state_dict() is None
    # load_ema_state_dict makes the owner's buffer, writes the trainable slots only and leaves the parameters alone
    sd = eng.state_dict()
    tr = [k for k, v in eng.slot.items() if v[0]]
    want = {k: torch.full_like(sd[k], 0.25) for k in sd}
    second.load_ema_state_dict(want)
    assert eng._ema is not None and second._ema is None
    got = second.ema_state_dict()
    assert list(got) == list(sd)
    for k in sd:
        assert torch.equal(got[k], want[k] if k in tr else sd[k]), k
        assert torch.equal(eng.state_dict()[k], sd[k])
