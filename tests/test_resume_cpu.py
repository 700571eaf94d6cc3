"""CPU side of checkpointing the optimiser state (--save_optimizer / --resume): optstate's packing between flat buffers and the
per-key format-1 dict on a made-up slot table, its errors, to_torch_adam_state against torch.optim.Adam(amsgrad=True) itself, the
flags, and the engine / TnrAdam surface on a CPU engine (no kernel is involved anywhere in saving or loading).  Every comparison
of saved against restored data is torch.equal."""
import pytest
import torch

import optstate as OS

# a slot table with what the engine's has: frozen entries in between (offsets of another buffer), groups that start 64-aligned,
# so gaps behind "b.bias" (70 .. 128) and behind "c.weight" (140 .. 192); n_train leaves a tail gap as well
SLOT = {"a.weight": (True, 0, 60, (6, 10)), "frozen.weight": (False, 0, 33, (3, 11)), "b.bias": (True, 64, 6, (6,)),
        "c.weight": (True, 128, 12, (3, 4)), "frozen.bias": (False, 64, 5, (5,)), "d": (True, 192, 1, (1, 1))}
N_TRAIN = 256
GAPS = [(60, 64), (70, 128), (140, 192), (193, 256)]


def _buffers(seed=0, gaps=0.0):
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(3):
        t = torch.randn(N_TRAIN, generator=g)
        for a, b in GAPS:
            t[a:b] = gaps
        out.append(t)
    return out


def _osd(state, **kw):
    return OS.make(kw.pop("dtype", "bf16"), kw.pop("step", 3), state, **kw)


def test_round_trip_on_a_table_with_gaps():
    m, v, vmax = _buffers()
    state = OS.unpack(SLOT, m, v, vmax)
    assert list(state) == ["a.weight", "b.bias", "c.weight", "d"] == [k for k, _, _, _ in OS.trainable_slots(SLOT)]
    for k, st in state.items():
        _, o, n, shp = SLOT[k]
        assert list(st) == list(OS.MOMENTS) == ["exp_avg", "exp_avg_sq", "max_exp_avg_sq"]
        for name, buf in zip(OS.MOMENTS, (m, v, vmax)):
            t = st[name]
            assert t.dtype == torch.float32 and t.device.type == "cpu" and tuple(t.shape) == shp
            assert torch.equal(t.reshape(-1), buf[o:o + n])
            assert t.data_ptr() != buf[o:o + n].data_ptr()           # a copy: a later step does not change what was saved
    back = OS.pack(SLOT, N_TRAIN, state)
    assert all(torch.equal(a, b) for a, b in zip(back, (m, v, vmax)))
    # whatever the source held between the slots, the packed buffers hold zeros there
    dirty = _buffers(gaps=7.0)
    back = OS.pack(SLOT, N_TRAIN, OS.unpack(SLOT, *dirty))
    for a, d in zip(back, dirty):
        for lo, hi in GAPS:
            assert float(a[lo:hi].abs().max()) == 0.0 and float(d[lo:hi].min()) == 7.0
        for k, (tr, o, n, _) in SLOT.items():
            if tr:
                assert torch.equal(a[o:o + n], d[o:o + n])
    # through torch.save / torch.load the dict keeps its bits and its key order
    import io
    f = io.BytesIO()
    torch.save(_osd(state, scaler=dict(mult=0.5, clean=1, run_of_skips=0, skipped=1, stamp=4, guard=[3, 1, 0, 0]), ema_updates=3), f)
    f.seek(0)
    got = torch.load(f)
    assert list(got) == ["format", "dtype", "step", "state", "scaler", "ema_updates", "dropout_calls"] and got["format"] == 1
    assert list(got["state"]) == list(state) and got["scaler"]["guard"] == [3, 1, 0, 0] and got["step"] == 3
    assert all(torch.equal(a, b) for a, b in zip(OS.pack(SLOT, N_TRAIN, got["state"]), (m, v, vmax)))


def test_errors_name_what_is_wrong():
    state = OS.unpack(SLOT, *_buffers())
    with pytest.raises(KeyError, match="missing key: c.weight"):
        OS.pack(SLOT, N_TRAIN, {k: v for k, v in state.items() if k != "c.weight"})
    with pytest.raises(KeyError, match="frozen.weight is not a trainable parameter"):
        OS.pack(SLOT, N_TRAIN, dict(state, **{"frozen.weight": state["d"]}))
    with pytest.raises(KeyError, match="nowhere is not a trainable parameter"):
        OS.pack(SLOT, N_TRAIN, dict(state, nowhere=state["d"]))
    bad = dict(state, **{"c.weight": dict(state["c.weight"], exp_avg_sq=torch.zeros(4, 3))})
    with pytest.raises(ValueError, match=r"c.weight: exp_avg_sq has shape \(4, 3\) != \(3, 4\)"):
        OS.pack(SLOT, N_TRAIN, bad)
    with pytest.raises(ValueError, match="unknown format 2"):
        OS.check_header(dict(_osd(state), format=2), "bf16")
    with pytest.raises(ValueError, match="unknown format None"):
        OS.check_header({}, "bf16")
    with pytest.raises(ValueError, match="saved under dtype bf16, this engine runs fp16"):
        OS.check_header(_osd(state), "fp16")
    OS.check_header(_osd(state), "bf16")
    with pytest.raises(KeyError, match="missing key: zzz"):
        OS.to_torch_adam_state(_osd(state), ["a.weight", "zzz"])


def test_to_torch_adam_state_continues_a_torch_run():
    """torch.optim.Adam(amsgrad=True), two tensors, five steps; its state after three steps goes into an osd (as the engine's flat
    buffers would hold it, through pack / unpack), through the helper into a FRESH torch optimiser, which takes the last two steps:
    the parameters equal the five-step run's bit for bit - "step" and the three moments mean what torch means by them."""
    names, shapes = ["a.weight", "c.weight"], [(6, 10), (3, 4)]
    slot = {k: SLOT[k] for k in names}
    g = torch.Generator().manual_seed(1)
    p0 = [torch.randn(s, generator=g) for s in shapes]
    grads = [[torch.randn(s, generator=g) for s in shapes] for _ in range(5)]

    def run(params, opt, steps):
        for s in steps:
            for p, gr in zip(params, grads[s]):
                p.grad = gr.clone()
            opt.step()

    mk = lambda ps: torch.optim.Adam(ps, lr=1e-2, betas=(0.9, 0.999), eps=1e-8, amsgrad=True)
    straight = [p.clone().requires_grad_() for p in p0]
    run(straight, mk(straight), range(5))
    first = [p.clone().requires_grad_() for p in p0]
    opt = mk(first)
    run(first, opt, range(3))
    st = opt.state_dict()["state"]
    assert all(float(st[i]["step"]) == 3.0 for i in range(2))
    flat = [torch.zeros(N_TRAIN) for _ in range(3)]
    for i, k in enumerate(names):
        _, o, n, _ = slot[k]
        for buf, name in zip(flat, OS.MOMENTS):
            buf[o:o + n] = st[i][name].reshape(-1)
    osd = _osd(OS.unpack(slot, *flat), step=3)
    half = OS.to_torch_adam_state(osd, names)
    assert list(half) == ["state"] and list(half["state"]) == [0, 1]
    assert all(list(half["state"][i]) == ["step", "exp_avg", "exp_avg_sq", "max_exp_avg_sq"] for i in range(2))
    second = [p.detach().clone().requires_grad_() for p in first]
    opt2 = mk(second)
    opt2.load_state_dict(dict(half, param_groups=opt2.state_dict()["param_groups"]))
    run(second, opt2, range(3, 5))
    assert all(torch.equal(a, b) for a, b in zip(second, straight))
    # ... and it discriminates: without the state, or with the step count lost, the last two steps end elsewhere
    cold = [p.detach().clone().requires_grad_() for p in first]
    run(cold, mk(cold), range(3, 5))
    assert not any(torch.equal(a, b) for a, b in zip(cold, straight))
    late = [p.detach().clone().requires_grad_() for p in first]
    opt3 = mk(late)
    opt3.load_state_dict(dict(OS.to_torch_adam_state(dict(osd, step=1), names), param_groups=opt3.state_dict()["param_groups"]))
    run(late, opt3, range(3, 5))
    assert not any(torch.equal(a, b) for a, b in zip(late, straight))
    # the reversed name order gives the reversed index order
    rev = OS.to_torch_adam_state(osd, names[::-1])
    assert torch.equal(rev["state"][0]["exp_avg"], osd["state"][names[1]]["exp_avg"])
    assert rev["state"][0]["exp_avg"].data_ptr() != osd["state"][names[1]]["exp_avg"].data_ptr()     # copies: torch updates them in place


def test_flags():
    import parameters
    a = parameters.parse_args([])
    assert a.resume is False and a.save_optimizer is False and a.start_epoch == 0
    with pytest.raises(ValueError, match="--resume True needs --load_ckpt_name"):
        parameters.parse_args(["--resume", "True"])
    b = parameters.parse_args(["--resume", "True", "--load_ckpt_name", "epoch-1.pt", "--save_optimizer", "True"])
    assert b.resume is True and b.save_optimizer is True
    parameters.parse_args(["--load_ckpt_name", "epoch-1.pt", "--start_epoch", "1"])           # as before: no --resume needed
    helps = {act.dest: act.help or "" for act in parameters.build_parser()._actions}
    for k in ("warmup_steps", "lr_decay_steps", "ema_warmup"):
        assert "not checkpointed" not in helps[k].lower() and "--save_optimizer" in helps[k] and "--resume" in helps[k], k
    assert not any("not checkpointed" in h.lower() for h in helps.values())
    import engine as E
    assert "not checkpointed" not in E.Engine.step.__doc__.lower() and "optimizer_state_dict" in E.Engine.step.__doc__


def test_run_py_refuses_resume_without_a_checkpoint_before_building_anything():
    import types
    import run
    with pytest.raises(ValueError, match="--resume True needs --load_ckpt_name"):
        run.train(types.SimpleNamespace(resume=True, load_ckpt_name=None))


def _cpu_engine(trainable=(0,), share=None):
    import engine as E
    cfg = E.EngineConfig(n_layers=1, trainable_layers=trainable, num_teachers=1)
    return E.Engine(cfg, device="cpu", max_batch=1, share=share)


def test_engine_surface_on_a_cpu_engine():
    """Save and load move data only, so the whole engine path runs on CPU buffers (fp16 engine, its scaler off without a GPU):
    whole-buffer equality after a round trip into a second engine, forwarding through share=, the counters, and the refusals."""
    eng = _cpu_engine()
    g = torch.Generator().manual_seed(2)
    for buf in (eng.adam_m, eng.adam_v, eng.adam_vmax):
        buf.copy_(torch.randn(eng.n_train, generator=g))
    used = torch.zeros(eng.n_train, dtype=torch.bool)
    for k, (tr, o, n, _) in eng.slot.items():
        if tr:
            used[o:o + n] = True
    assert bool((~used).any())                                       # the real table has gaps
    for buf in (eng.adam_m, eng.adam_v, eng.adam_vmax):
        buf[~used] = 0.0
    eng.step_count, eng.drop_calls = 7, 5
    before = [b.clone() for b in (eng.flat[True], eng.flat[False], eng.flat_g, eng.adam_m, eng.adam_v, eng.adam_vmax)]
    second = _cpu_engine(share=eng)
    osd = second.optimizer_state_dict()                              # forwards to the owner
    assert all(torch.equal(a, b) for a, b in zip(before, (eng.flat[True], eng.flat[False], eng.flat_g, eng.adam_m, eng.adam_v, eng.adam_vmax)))
    assert osd["format"] == 1 and osd["dtype"] == "fp16" and osd["step"] == 7 and osd["dropout_calls"] == 5
    assert osd["scaler"] is None and osd["ema_updates"] is None
    assert list(osd["state"]) == [k for k, v in eng.slot.items() if v[0]]
    assert all(tuple(osd["state"][k]["exp_avg"].shape) == tuple(eng.shapes[k]) for k in osd["state"])
    other = _cpu_engine()
    other.adam_m.fill_(3.0)                                          # stale state, gaps included, must go
    other_share = _cpu_engine(share=other)
    other_share.load_optimizer_state_dict(osd)
    assert torch.equal(other.adam_m, eng.adam_m) and torch.equal(other.adam_v, eng.adam_v) and torch.equal(other.adam_vmax, eng.adam_vmax)
    assert other.step_count == 7 and other.drop_calls == 5 and other._ema is None and other.ema_updates == 0
    # with an average: its count travels
    eng.load_ema_state_dict(eng.state_dict())
    eng.ema_updates = 4
    assert eng.optimizer_state_dict()["ema_updates"] == 4
    other.load_optimizer_state_dict(eng.optimizer_state_dict())
    assert other.ema_updates == 4
    # refusals: nothing is written by a load that fails
    keep = other.adam_m.clone()
    for bad, err, msg in ((dict(osd, format=9), ValueError, "unknown format 9"),
                          (dict(osd, dtype="bf16"), ValueError, "saved under dtype bf16, this engine runs fp16"),
                          (dict(osd, state={k: v for k, v in list(osd["state"].items())[1:]}), KeyError, "missing key: " + list(osd["state"])[0])):
        with pytest.raises(err, match=msg):
            other.load_optimizer_state_dict(bad)
        assert torch.equal(other.adam_m, keep) and other.step_count == 7
    frozen = _cpu_engine(trainable=())
    with pytest.raises(KeyError, match="is not a trainable parameter of this engine"):
        frozen.load_optimizer_state_dict(osd)
    with pytest.raises(KeyError, match="missing key"):
        other.load_optimizer_state_dict(frozen.optimizer_state_dict())
    eng._acc_held = 1
    with pytest.raises(AssertionError, match="accumulation window"):
        second.optimizer_state_dict()
    with pytest.raises(AssertionError, match="accumulation window"):
        second.load_optimizer_state_dict(osd)


class _StubModel:
    def __init__(self):
        self.loaded, self._micro = [], None
        self.engine = self

    def accum_reset(self):
        self.loaded.append("accum_reset")

    def optimizer_state_dict(self):
        return {"format": 1}

    def load_optimizer_state_dict(self, osd):
        self.loaded.append(osd)

    def step(self, lr, **kw):
        pass


def test_tnr_adam_state_dict_refuses_inside_a_window_and_load_resets_it():
    from model_bert import TnrAdam
    m = _StubModel()
    opt = TnrAdam(m, 1e-4, grad_accum_steps=2)
    assert opt.state_dict() == {"format": 1}
    opt.step()
    assert opt._pos == 1
    with pytest.raises(RuntimeError, match="inside an accumulation window"):
        opt.state_dict()
    with pytest.raises(RuntimeError, match="inside an accumulation window"):
        opt.load_state_dict({"format": 1})
    opt.step()
    opt.load_state_dict({"format": 1})
    assert m.loaded == [{"format": 1}, "accum_reset"] and opt._pos == 0 and m._micro == (0, 2)
