"""CPU side of gradient accumulation (--grad_accum_steps): TnrAdam's window logic against a stub model and engine that record
their calls, and the flag."""
import pytest


class _StubEngine:
    def __init__(self):
        self.calls, self.resets = [], 0

    def step(self, lr, **kw):
        self.calls.append((lr, kw))

    def accum_reset(self):
        self.resets += 1


class _StubModel:
    strict_grad_scale = False

    def __init__(self):
        self.engine = _StubEngine()
        self._micro = None


class _Sync:
    scale = 0.25                      # four ranks


def _drive(K, n, sync=None, **kw):
    """n step() calls -> (model, the indices of the calls that reached the engine, the (j, K) backward would have been handed
    before each call)"""
    from model_bert import TnrAdam
    m = _StubModel()
    opt = TnrAdam(m, 1e-4, sync, grad_accum_steps=K, **kw)
    reached, seen = [], []
    for i in range(n):
        seen.append(m._micro)
        before = len(m.engine.calls)
        opt.zero_grad()
        opt.step()
        if len(m.engine.calls) > before:
            reached.append(i)
    return m, opt, reached, seen


@pytest.mark.parametrize("K,want", [(1, [0, 1, 2, 3, 4, 5, 6]), (2, [1, 3, 5]), (3, [2, 5])])
def test_which_of_seven_steps_reach_the_engine(K, want):
    m, opt, reached, seen = _drive(K, 7)
    assert reached == want
    if K == 1:
        assert seen == [None] * 7 and m._micro is None                 # nothing is published: backward makes today's call
    else:
        assert seen == [(i % K, K) for i in range(7)] and m._micro == (7 % K, K)
    for lr, kw in m.engine.calls:
        assert lr == 1e-4 and set(kw) == {"grad_scale", "lr_bert", "lr_news_head", "sync"} and kw["sync"] is None
        assert kw["grad_scale"] == 1.0 / K


@pytest.mark.parametrize("K", [1, 2, 3])
def test_grad_scale_is_the_sync_scale_over_K_and_the_rest_is_passed_as_before(K):
    s = _Sync()
    m, opt, reached, _ = _drive(K, K, s, max_grad_norm=0.5, weight_decay=0.01, ema_decay=0.9, pretrain_lr=1e-5)
    (lr, kw), = m.engine.calls
    assert kw["grad_scale"] == 0.25 / K and kw["sync"] is s and kw["lr_bert"] == 1e-5 and kw["lr_news_head"] is None
    assert kw["max_grad_norm"] == 0.5 and kw["weight_decay"] == 0.01 and kw["ema_decay"] == 0.9 and kw["ema_warmup"] is False
    assert set(kw) == {"grad_scale", "lr_bert", "lr_news_head", "sync", "max_grad_norm", "weight_decay", "warmup_steps",
                       "lr_decay_steps", "ema_decay", "ema_warmup"}


def test_reset_window_mid_window():
    m, opt, reached, _ = _drive(3, 2)                                   # two micro-batches into a window of three
    assert reached == [] and m._micro == (2, 3) and m.engine.resets == 0
    opt.reset_window()
    assert m._micro == (0, 3) and m.engine.resets == 1 and not m.engine.calls
    for i in range(3):
        assert m._micro == (i, 3)
        opt.step()
    assert len(m.engine.calls) == 1 and m._micro == (0, 3)
    # K = 1: nothing to reset, nothing published, the engine is not touched
    m1, opt1, _, _ = _drive(1, 1)
    opt1.reset_window()
    assert m1._micro is None and m1.engine.resets == 0 and len(m1.engine.calls) == 1


def test_strict_grad_scale_and_bad_K_raise():
    from model_bert import TnrAdam
    m = _StubModel()
    m.strict_grad_scale = True
    with pytest.raises(ValueError, match="strict_grad_scale"):
        TnrAdam(m, 1e-4, grad_accum_steps=2)
    TnrAdam(m, 1e-4, grad_accum_steps=1)                                # fine without accumulation
    with pytest.raises(ValueError, match="at least 1"):
        TnrAdam(_StubModel(), 1e-4, grad_accum_steps=-2)
    assert TnrAdam(None, 1e-4).grad_accum_steps == 1


def test_flag_parses_with_default_1_and_rejects_0(capsys):
    import parameters
    assert parameters.parse_args([]).grad_accum_steps == 1
    assert parameters.parse_args(["--grad_accum_steps", "4"]).grad_accum_steps == 4
    for bad in ("0", "-1", "1.5"):
        with pytest.raises(SystemExit):
            parameters.parse_args(["--grad_accum_steps", bad])
    assert "grad_accum_steps" in capsys.readouterr().err
    text = " ".join(parameters.build_parser().format_help().split()).replace("- ", "-")     # argparse wraps behind hyphens
    for phrase in ("effective batch", "count updates, not batches", "one gradient all-reduce per update", "partial window"):
        assert phrase in text, phrase


def test_engine_without_accumulation_allocates_nothing_new():
    import engine as E
    eng = E.Engine(E.EngineConfig(n_layers=1, trainable_layers=(0,), num_teachers=1), device="cpu", max_batch=1)
    second = E.Engine(eng.cfg, device="cpu", max_batch=1, share=eng)
    assert eng._acc is None and second._acc is None and eng._acc_held == 0
    acc = second._acc_buffer()                                          # made by (and for) the engine that owns flat_g
    assert eng._acc is acc and second._acc is None and acc.shape == eng.flat_g.shape and acc.dtype == eng.flat_g.dtype
    eng._acc_held = 1
    with pytest.raises(AssertionError, match="inside an accumulation window"):
        second.step(1e-4)
    second.accum_reset()
    assert eng._acc_held == 0
