"""What Engine.step sends to the device, as data: every tnr_hip.call with its arguments, every wait on a GradSync and every
queued read-back into pinned memory, in order, for a list of scenarios that covers each mode of the step without a sync, with
collectives in flight and with collectives that have all landed.  tools/step_trace.py records the list into
tests/golden/step_trace.json.gz; tests/test_step_trace_gpu.py replays it on the code as it is and compares.

An entry is one of
  ["step", s]                step number s of the scenario begins
  ["call", name, arg, ...]   tnr_hip.call(name, *args)
  ["wait_bucket", b]         sync.wait_bucket(b)
  ["wait"]                   sync.wait()
  ["record", label]          dst.copy_(src, non_blocking=True) into pinned memory: a read-back of `label` (the scaler's guard word,
                             the clip floats, the trust table)
Arguments are normalised so that the trace depends on neither the machine nor the allocator: a tensor is [label, byte offset]
with the label of the named buffer its data_ptr() lies in (labels(): the flat buffers, Adam's moments, the owner's lazily made
state, the scaler's guard, the shadow tables and copies; a pointer in none of them raises), None stays None, an int stays an
int, a float is float.hex() (the arguments are host doubles: exact).

Every scenario runs on the 2-layer, 2-teacher engine of tests/test_grad_clip_gpu.py with its fill() gradients and no forward
pass.  Only attributes that every version of the step keeps are touched, so the recording tool runs on any commit."""
import gzip
import json
import math

import pytest
import torch

import tnr_hip as T
from test_grad_clip_gpu import DEV, RATES, FakeSync, fill, gen, make

VERSION = 1
DTYPES = ("fp16", "bf16")


class TracedSync(FakeSync):
    """FakeSync that writes its waits into the trace.  landed: every collective has completed already (pending is empty)."""

    def __init__(self, ranges, log, landed=False):
        FakeSync.__init__(self, ranges)
        self.log = log
        if landed:
            self.pending.clear()

    def wait_bucket(self, b):
        self.log.append(["wait_bucket", b])
        FakeSync.wait_bucket(self, b)

    def wait(self):
        self.log.append(["wait"])
        for b in list(self.pending):
            FakeSync.wait_bucket(self, b)


def labels(eng):
    """[(label, tensor)] of every buffer a step may name, looked up on the engine that owns flat_g."""
    own = eng._clip_owner
    out = [("flat", own.flat[True]), ("flat_g", own.flat_g), ("adam_m", own.adam_m), ("adam_v", own.adam_v),
           ("adam_vmax", own.adam_vmax), ("ema", own._ema), ("decay_map", own._decay_map), ("acc", own._acc),
           ("guard", own.scaler.guard), ("desc_train.desc", own.desc_train[0]), ("desc_train.start", own.desc_train[3]),
           ("sh_a1", own.sh_a1), ("sh_a1T", own.sh_a1T)]
    for what, st in (("clip", own._clip_state), ("lamb", own._lamb_state)):
        if st is not None:
            out += [("%s.%s" % (what, k), v) for k, v in sorted(vars(st).items()) if isinstance(v, torch.Tensor)]
    for l, d in enumerate(own.sh):
        out += [("sh%d.%s" % (l, k), v) for k, v in sorted(d.items())]
    return [(k, v) for k, v in out if v is not None]


def label_of(eng, t):
    p = t.data_ptr()
    for name, buf in labels(eng):
        lo = buf.data_ptr()
        if lo <= p < lo + buf.numel() * buf.element_size():
            return [name, p - lo]
    raise AssertionError("a tensor of %d x %s at %#x lies in no named buffer" % (t.numel(), t.dtype, p))


def norm_arg(eng, a):
    if a is None or (isinstance(a, int) and not isinstance(a, bool)):
        return a
    if isinstance(a, float):
        return a.hex()
    if isinstance(a, torch.Tensor):
        return label_of(eng, a)
    raise AssertionError("argument of type %s" % type(a).__name__)


def record(eng, log, mp):
    """Route tnr_hip.call and the non-blocking copies into pinned memory through `log` until `mp` (a pytest.MonkeyPatch) undoes it."""
    real_call, real_copy = T.call, torch.Tensor.copy_

    def call(name, *args):
        log.append(["call", name] + [norm_arg(eng, a) for a in args])
        return real_call(name, *args)

    def copy_(dst, src, non_blocking=False):
        if non_blocking and dst.is_pinned():
            log.append(["record", label_of(eng, src)[0]])
        return real_copy(dst, src, non_blocking=non_blocking)
    mp.setattr(T, "call", call)
    mp.setattr(torch.Tensor, "copy_", copy_)


def _modes(n_train):
    clip = 0.6 * 0.5 * 1e-3 * math.sqrt(n_train)            # clips fill(1e-3) gradients under grad_scale 0.5
    three = dict(lr_bert=RATES[1], lr_news_head=RATES[2])
    adamw = dict(weight_decay=0.01, warmup_steps=3, lr_decay_steps=10)
    ema = dict(ema_decay=0.999, ema_warmup=True)
    return [("plain", three),
            ("plain_one_rate_adam", dict(amsgrad=False)),          # one rate: the three ranges merge into one launch
            ("clip", dict(three, max_grad_norm=clip)),
            ("adamw", dict(three, **adamw)),
            ("ema", dict(three, **ema)),
            ("clip_decay_ema", dict(three, max_grad_norm=clip, weight_decay=0.01, **ema)),
            ("lamb", dict(three, lamb=True)),
            ("lamb_all", dict(three, lamb=True, max_grad_norm=clip, **adamw, **ema))]


def scenarios():
    """[name]: <dtype>-<mode>-<sync> with sync one of none / pending / landed, the two overflow runs and the share= runs."""
    out = []
    for dt in DTYPES:
        for mode, _ in _modes(64):
            out += ["%s-%s-%s" % (dt, mode, s) for s in ("none", "pending")]
            if mode in ("plain", "clip", "lamb"):
                out.append("%s-%s-landed" % (dt, mode))
        out.append("%s-share_lamb_clip_ema-none" % dt)
    return out + ["fp16-overflow-none", "fp16-overflow-pending"]


def run(name):
    """Run one scenario on a fresh engine and return its trace."""
    dt, mode, how = name.split("-")
    eng = own = make(dt)
    kw = dict(_modes(own.n_train)).get(mode)
    steps, bad = 2, None
    if mode == "share_lamb_clip_ema":
        import engine as E
        eng = E.Engine(own.cfg, DEV, max_batch=2, dtype=dt, share=own)
        kw = dict(lr_bert=RATES[1], lr_news_head=RATES[2], lamb=True, max_grad_norm=dict(_modes(own.n_train))["clip"]["max_grad_norm"],
                  ema_decay=0.999)
    elif mode == "overflow":
        kw = dict(_modes(own.n_train))["adamw"]
        kw = dict(kw, ema_decay=0.999, ema_warmup=True)
        steps, bad = 5, 1
    ranges = own.bucket_ranges()
    g, log = gen(), []
    torch.cuda.synchronize()
    with pytest.MonkeyPatch.context() as mp:
        record(eng, log, mp)
        for s in range(steps):
            fill(own, g, 1e-3)                                     # (its copy_ is a blocking one: not a read-back)
            if s == bad:
                own.flat_g[ranges[-1][1] - 1] = float("inf")       # the last element of the bucket that lands last
            sync = None if how == "none" else TracedSync(ranges, log, landed=how == "landed")
            log.append(["step", s])
            eng.step(RATES[0], grad_scale=0.5, sync=sync, **kw)
    torch.cuda.synchronize()
    if eng is not own:
        assert eng._clip_state is None and eng._lamb_state is None and eng._ema is None and eng._decay_map is None
        assert own._clip_state is not None and own._lamb_state is not None and own._ema is not None
    if bad is not None:
        own.scaler.drain(own)
        assert own.scaler.skipped == 1 and own.step_count == steps - 1
    return log


def dumps(traces):
    """Canonical text of {scenario: trace}."""
    return json.dumps({"version": VERSION, "scenarios": traces}, sort_keys=True, separators=(",", ":"))


def save(path, traces):
    with open(path, "wb") as f, gzip.GzipFile(fileobj=f, mode="wb", mtime=0, filename="") as z:
        z.write(dumps(traces).encode())


def load(path):
    with gzip.open(path, "rb") as z:
        d = json.loads(z.read().decode())
    assert d["version"] == VERSION
    return d["scenarios"]
