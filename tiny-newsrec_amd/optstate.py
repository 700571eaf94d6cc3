"""Packing of the optimiser state between the engine's flat fp32 buffers and a per-key checkpoint (format 1).

The engine keeps Adam's moments in three flat buffers laid out by its slot table {key: (trainable, offset, numel, shape)}; a
checkpoint keeps them per trainable key, shaped like the parameter, under the names torch.optim.Adam(amsgrad=True).state_dict()
gives its per-parameter state (exp_avg, exp_avg_sq, max_exp_avg_sq) - independent of the table's alignment gaps and readable beside
model_state_dict.  Host side only: torch tensors in, torch CPU tensors out; nothing here knows the HIP library.

    {"format": 1, "dtype": "fp16" | "bf16",
     "step": int,                         # updates TAKEN (Engine.step_count with the fp16 scaler drained)
     "state": {key: {"exp_avg": fp32, "exp_avg_sq": fp32, "max_exp_avg_sq": fp32}},       # every trainable key, table order
     "scaler": None | {"mult", "clean", "run_of_skips", "skipped", "stamp", "guard": [4 ints]},
     "ema_updates": None | int,
     "dropout_calls": int}                # Stage1Engine: [title, body]
"""
import torch

FORMAT = 1
MOMENTS = ("exp_avg", "exp_avg_sq", "max_exp_avg_sq")       # adam_m, adam_v, adam_vmax
SCALER_FIELDS = ("mult", "clean", "run_of_skips", "skipped", "stamp")


def trainable_slots(slot):
    """[(key, offset, numel, shape)] of the trainable keys, in the table's order."""
    return [(k, o, n, tuple(shp)) for k, (tr, o, n, shp) in slot.items() if tr]


def unpack(slot, m, v, vmax):
    """Flat buffers (any device) -> {key: {"exp_avg", "exp_avg_sq", "max_exp_avg_sq"}} of fp32 CPU tensors that own their memory,
    one entry per trainable key in the table's order.  Slices are copied as they are (device-to-host copies, no kernel)."""
    out = {}
    for k, o, n, shp in trainable_slots(slot):
        out[k] = {name: buf[o:o + n].detach().to("cpu", copy=True).view(shp) for name, buf in zip(MOMENTS, (m, v, vmax))}
    return out


def pack(slot, n_train, state):
    """{key: {...}} -> (m, v, vmax): three fp32 CPU buffers of n_train elements, zero between the slots (what the update kernels
    keep there: the gaps' gradients are zero).  KeyError for a trainable key that is missing and for a key that is not trainable
    here, ValueError for a tensor whose shape is not its parameter's."""
    want = trainable_slots(slot)
    names = {k for k, _, _, _ in want}
    for k, _, _, _ in want:
        if k not in state:
            raise KeyError("optimiser state: missing key: %s" % k)
    for k in state:
        if k not in names:
            raise KeyError("optimiser state: %s is not a trainable parameter of this engine" % k)
    flat = [torch.zeros(int(n_train), dtype=torch.float32) for _ in MOMENTS]
    for k, o, n, shp in want:
        for name, buf in zip(MOMENTS, flat):
            if name not in state[k]:
                raise KeyError("optimiser state: %s has no %s" % (k, name))
            t = state[k][name]
            t = t if isinstance(t, torch.Tensor) else torch.as_tensor(t)
            if tuple(t.shape) != shp:
                raise ValueError("optimiser state: %s: %s has shape %s != %s" % (k, name, tuple(t.shape), shp))
            buf[o:o + n].view(shp).copy_(t.detach().to("cpu", torch.float32))
    return tuple(flat)


def check_header(osd, dtype):
    """ValueError for a format this code does not read and for a state saved under the other 16-bit type (the loss scaler's state
    is not portable and no cross-dtype continuation is promised)."""
    if osd.get("format") != FORMAT:
        raise ValueError("optimiser state: unknown format %r (this build reads format %d)" % (osd.get("format"), FORMAT))
    if osd.get("dtype") != dtype:
        raise ValueError("optimiser state: saved under dtype %s, this engine runs %s" % (osd.get("dtype"), dtype))


def make(dtype, step, state, scaler=None, ema_updates=None, dropout_calls=0):
    """The format-1 dict from its parts."""
    return {"format": FORMAT, "dtype": dtype, "step": int(step), "state": state, "scaler": scaler,
            "ema_updates": None if ema_updates is None else int(ema_updates), "dropout_calls": dropout_calls}


def rekey(osd, fn):
    """The same dict with every key of "state" mapped through fn (order kept)."""
    return dict(osd, state={fn(k): v for k, v in osd["state"].items()})


def to_torch_adam_state(osd, names):
    """The "state" half of torch.optim.Adam(amsgrad=True).state_dict() for the parameters `names`, in that order:
    {"state": {i: {"step", "exp_avg", "exp_avg_sq", "max_exp_avg_sq"}}} - "step" is the number of updates taken (a float32
    scalar tensor, as torch keeps it), the three moments are torch's of the same names.  With that optimiser's own param_groups it
    is a dict its load_state_dict() takes."""
    out = {}
    for i, k in enumerate(names):
        if k not in osd["state"]:
            raise KeyError("optimiser state: missing key: %s" % k)
        st = {"step": torch.tensor(float(osd["step"]), dtype=torch.float32)}
        for name in MOMENTS:
            st[name] = osd["state"][k][name].detach().clone()
        out[i] = st
    return {"state": out}
