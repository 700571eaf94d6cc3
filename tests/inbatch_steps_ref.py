"""Shared by tests/test_inbatch_steps_ref_cpu.py and tests/test_inbatch_steps_gpu.py: the schedules of unlike steps that one long-lived
Engine is driven through with in-batch negatives switched on and off.  Imports no GPU module.

What the option adds to an engine is state that crosses calls: Engine._ib_on is written by forward and read by backward, the
buffers of Engine._inbatch follow the workspace's re-lay, dz holds raw logits between the loss kernel's two phases.  As in
tests/history_ref.py, a schedule visits the step pairs at which that state could go wrong, and the GPU test compares every step,
bit for bit, with the same step on a fresh engine that has that step's weights, switches and loss-scale multiplier.

Model, weights and news tables: history_ref / variants_ref ("att" unless a record names another); feeds: inbatch_ref.engine_feed
("e3", "e5", "e5b": B = 3, 5, 5, ids that collide under all five rules).

A record (step()): feed, on, plan, feed form, micro (j, K), dropout (p_hidden, p_attn, seed) or None, the fp16 scaler multiplier,
`only` (a 16-bit type the record is for), backward (False: a forward alone), `mid`: a forward-only path run between the step's
forward and its backward, `pre`: actions in front of the step."""
import inbatch_ref as R

LR = 1e-3
DROP = (0.1, 0.1, 4242)
PATHS = ("rank_metrics", "encode_table", "user_vectors")


def step(feed, on, plan=False, form="idx", micro=None, drop=None, mult=1.0, only=None, backward=True, mid=None, pre=()):
    assert feed in R._ENGINE and form in ("idx", "tok") and (mid is None or mid in PATHS)
    assert backward or (micro is None and mid is None)
    return dict(feed=feed, B=R._ENGINE[feed][0], on=bool(on), plan=plan, form=form, micro=micro, drop=drop, mult=mult, only=only,
                backward=backward, mid=mid, pre=tuple(pre))


SCHEDULES = {
    # the switch itself: Engine._ib_on between a forward and the backward that reads it
    "toggle": [
        step("e5", True),
        step("e5b", False),
        step("e5", True),
        step("e5b", True, backward=False),                 # an on forward that no backward follows ...
        step("e5", False),                                 # ... then an off step: its flat_g must be the off engine's
        step("e5b", False, backward=False),
        step("e5", True),                                  # and the reverse
    ],
    # forward-only paths inside an on step, the short batch under a plan, the other feed form
    "paths": [
        step("e5", True, mid="rank_metrics", pre=[("encode_table",)]),
        step("e5b", True, mid="encode_table"),
        step("e5", True, mid="user_vectors"),
        step("e3", True, plan=True),                       # B = 5 -> 3: the buffers follow the re-lay; a plan on the short step only
        step("e5b", True),                                 # ... and back
        step("e5", True, form="tok"),                      # token feed after indexed feed
        step("e5", True),
    ],
    # dropout toggled, windows of unlike micro-batches, weights that move
    "moving": [
        step("e5", True),
        step("e5", True, drop=DROP),
        step("e5b", True, drop=DROP),
        step("e5", True),
        step("e5", True, micro=(0, 2)),
        step("e5b", False, micro=(1, 2)),
        step("e5", False, micro=(0, 2)),
        step("e5b", True, micro=(1, 2)),
        step("e5b", True, pre=[("step", LR)]),
        step("e5", False, pre=[("step", LR)]),
        step("e5", True),
    ],
    # fp16: the loss scale moves under an engine that has run on steps at another
    "scale": [
        step("e5", True, only="fp16"),
        step("e5", True, mult=0.5, only="fp16"),
        step("e5b", True, mult=2.0, only="fp16"),
        step("e5", True, mult=1.0, only="fp16"),
    ],
}


def windows(schedule, dtype):
    """The schedule's records for a 16-bit type, accumulation windows kept together: a list of lists of records."""
    recs = [r for r in schedule if r["only"] in (None, dtype)]
    out, i = [], 0
    while i < len(recs):
        k = recs[i]["micro"][1] if recs[i]["micro"] else 1
        assert [r["micro"] for r in recs[i:i + k]] == ([(j, k) for j in range(k)] if k > 1 else [None])
        out.append(recs[i:i + k])
        i += k
    return out


def pairs(schedule):
    """The step pairs a schedule visits, read back from its records as the names REQUIRED lists."""
    seen = set()
    sw = lambda r: "on" if r["on"] else "off"
    for i, r in enumerate(schedule):
        p = schedule[i - 1] if i else None
        q = schedule[i - 2] if i > 1 else None
        if r["mid"] and r["on"]:
            seen.add("on forward, %s, backward" % r["mid"])
        if any(a[0] == "step" for a in r["pre"]) and p is not None and p["backward"]:
            seen.add("%s after step() moved the weights" % sw(r))
        if r["micro"] and r["micro"][0] == 1 and p["micro"] == (0, 2):
            seen.add("window %s, %s" % (sw(p), sw(r)))
        if p is None or r["micro"] or p["micro"]:
            continue
        if p["backward"] and r["backward"]:
            seen.add("%s -> %s" % (sw(p), sw(r)))
            if q is not None and q["backward"] and not q["micro"]:
                seen.add("%s -> %s -> %s" % (sw(q), sw(p), sw(r)))
        if not p["backward"] and r["backward"]:
            seen.add("%s forward alone -> %s step" % (sw(p), sw(r)))
        if p["on"] and r["on"] and p["backward"] and r["backward"]:
            if (p["B"], r["B"]) == (5, 3) and r["plan"] and not p["plan"]:
                seen.add("B 5 -> 3 under a plan")
            if (p["B"], r["B"]) == (3, 5) and p["plan"] and not r["plan"] and q is not None and q["B"] == 5:
                seen.add("B 3 -> 5")
            if (p["form"], r["form"]) == ("idx", "tok"):
                seen.add("token feed after indexed feed")
            if not p["drop"] and r["drop"]:
                seen.add("dropout switched on")
            if p["drop"] and r["drop"]:
                seen.add("dropout stays on")
            if p["drop"] and not r["drop"]:
                seen.add("dropout switched off")
            if p["mult"] != r["mult"]:
                seen.add("scale %g -> %g" % (p["mult"], r["mult"]))
    return seen


REQUIRED = {
    "toggle": {"on -> off -> on", "on forward alone -> off step", "off forward alone -> on step"},
    "paths": {"on forward, rank_metrics, backward", "on forward, encode_table, backward", "on forward, user_vectors, backward",
              "B 5 -> 3 under a plan", "B 3 -> 5", "token feed after indexed feed"},
    "moving": {"dropout switched on", "dropout stays on", "dropout switched off", "window on, off", "window off, on",
               "on after step() moved the weights", "off after step() moved the weights"},
    "scale": {"scale 1 -> 0.5", "scale 0.5 -> 2", "scale 2 -> 1"},
}
