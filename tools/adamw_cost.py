"""What --weight_decay / --warmup_steps / --lr_decay_steps cost: the device time of Engine.step with them off, with a schedule
only, with decay + schedule, and with decay + schedule + clipping (beside clipping alone, its own baseline), fp16 and bf16, in ONE
process on one GPU at bench.py's headline shape (4 layers, (2, 3) trainable, 4 teachers, B = 32).

flat_g is filled once with N(0, 1e-3^2) (no forward: the optimiser step does not care where its gradient came from); every
Engine.step is bracketed with a pair of events, as bench.py's step_breakdown_ms brackets its calls, so a figure is the time from
the step's first kernel to the end of the weight-copy refresh, launch gaps included.  The variants alternate in rounds within the
process, and each reports median and the 10th / 90th percentile over all its steps: compare differences against that spread.  The
derived expectation: the update moves 36 n bytes per launch (5 reads, 4 writes of 4 bytes), the decay map adds n / 8: + 0.35 %.
The schedule is given a long warmup so that no variant ever runs at rate 0 or past its end.  EXPERIMENTS.md records the output.

    python tools/adamw_cost.py [--rounds 6] [--steps 40] [--batch 32]      -> one JSON line"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tiny-newsrec_amd"))
sys.path.insert(0, ROOT)

import numpy as np   # noqa: E402
import torch         # noqa: E402


def stats(us):
    us = np.asarray(us, np.float64)
    return {"median_us": round(float(np.median(us)), 1), "p10_us": round(float(np.percentile(us, 10)), 1),
            "p90_us": round(float(np.percentile(us, 90)), 1), "n": int(us.size)}


def timed(fn, n):
    """n calls of fn, each between two events on the current stream -> microseconds (one synchronise at the end)."""
    ev = []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        ev.append((e0, e1))
    torch.cuda.synchronize()
    return [1e3 * a.elapsed_time(b) for a, b in ev]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--steps", type=int, default=40, help="steps per variant and round")
    ap.add_argument("--batch", type=int, default=32)
    a = ap.parse_args()
    import engine as E
    import hashinit
    from schema import FULL, state_shapes
    if not torch.cuda.is_available():
        raise SystemExit("tools/adamw_cost.py measures on the GPU: none found")
    dev, seed = "cuda:0", 1234
    torch.cuda.set_device(0)
    cfg = E.EngineConfig()
    sd = hashinit.init_state_dict(seed, state_shapes(FULL, cfg.n_layers, cfg.D, cfg.T))
    out = {"batch": a.batch, "rounds": a.rounds, "steps_per_round": a.steps, "step": {}}
    for dtype in ("fp16", "bf16"):
        eng = E.Engine(cfg, dev, max_batch=a.batch, dtype=dtype)
        eng.load_state_dict(sd)
        eng.flat_g.copy_(torch.randn(eng.n_train, device=dev, generator=torch.Generator(device=dev).manual_seed(5)) * 1e-3)
        pos = 0
        for s_, e_ in sorted(eng.bucket_ranges()) + [(eng.n_train, eng.n_train)]:       # alignment gaps hold zeros after a backward
            eng.flat_g[pos:s_].zero_()
            pos = max(pos, e_)
        norm = 1e-3 * float(np.sqrt(eng.n_train))
        sched = {"warmup_steps": 1000000, "lr_decay_steps": 2000000}
        variants = {"off": {}, "schedule": dict(sched), "decay_schedule": dict(sched, weight_decay=0.01),
                    "clip": {"max_grad_norm": 0.5 * norm}, "decay_schedule_clip": dict(sched, weight_decay=0.01, max_grad_norm=0.5 * norm)}
        us = {k: [] for k in variants}
        for k, kw in variants.items():                                              # warm-up: every variant's kernels and buffers
            timed(lambda: eng.step(1e-4, **kw), 5)
        for _ in range(a.rounds):
            for k, kw in variants.items():
                us[k] += timed(lambda: eng.step(1e-4, **kw), a.steps)
        r = {k: stats(v) for k, v in us.items()}
        for k, base in (("schedule", "off"), ("decay_schedule", "off"), ("decay_schedule_clip", "off"), ("decay_schedule_clip", "clip")):
            r[k]["over_" + base] = round(r[k]["median_us"] / r[base]["median_us"], 4)
            r[k]["inside_%s_p10_p90" % base] = bool(r[base]["p10_us"] <= r[k]["median_us"] <= r[base]["p90_us"])
        r["n_train"], r["gradient_MB"] = int(eng.n_train), round(4e-6 * eng.n_train, 1)
        r["decay_map_KB"] = round(eng._decay_map.numel() * 4e-3, 1)
        r["decayed_elements"] = int(np.unpackbits(E.decay_words(eng.slot, eng.n_train).view(np.uint8)).sum())
        r["derived_extra_bytes"] = round((eng.n_train / 8.0) / (36.0 * eng.n_train), 5)
        out["step"][dtype] = r
        del eng
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
