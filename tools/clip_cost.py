"""What --max_grad_norm costs: the device time of Engine.step with clipping off and on, fp16 and bf16, in ONE process on one GPU at
bench.py's headline shape (4 layers, (2, 3) trainable, 4 teachers, B = 32); and, as the yardstick of the same run, the plain
non-finite scan (tnr_grad_nonfinite_scan) beside the fused one (tnr_grad_sumsq_scan with a guard) over the whole flat gradient.

flat_g is filled once with N(0, 1e-3^2) (no forward: the optimiser step does not care where its gradient came from); every
Engine.step is bracketed with a pair of events, as bench.py's step_breakdown_ms brackets its calls, so a figure is the time from
the step's first kernel to the end of the weight-copy refresh, launch gaps included.  The variants alternate in rounds within the
process, and each reports median and the 10th / 90th percentile over all its steps: compare differences against that spread.  The
gradient (59 MB) fits the chip's last-level cache and is re-read every step, here as in training, where the backward has just
written it.  EXPERIMENTS.md records the output.

    python tools/clip_cost.py [--rounds 6] [--steps 40] [--batch 32]      -> one JSON line"""
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
    import tnr_hip as T
    from schema import FULL, state_shapes
    if not torch.cuda.is_available():
        raise SystemExit("tools/clip_cost.py measures on the GPU: none found")
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
        variants = {"off": {}, "on_clipping": {"max_grad_norm": 0.5 * norm}, "on_not_clipping": {"max_grad_norm": 2.0 * norm}}
        us = {k: [] for k in variants}
        for k, kw in variants.items():                                              # warm-up: every variant's kernels and buffers
            timed(lambda: eng.step(1e-4, **kw), 5)
        for _ in range(a.rounds):
            for k, kw in variants.items():
                us[k] += timed(lambda: eng.step(1e-4, **kw), a.steps)
        r = {k: stats(v) for k, v in us.items()}
        r["n_train"], r["gradient_MB"] = int(eng.n_train), round(4e-6 * eng.n_train, 1)
        r["grad_norm_last"] = [round(x, 6) for x in eng.grad_norm()]
        out["step"][dtype] = r
        if dtype == "fp16":
            # the yardstick, same process: one launch over the whole gradient, plain scan / fused scan (guard given) / fused scan
            # without a guard (bf16's), alternating
            guard = torch.zeros(4, dtype=torch.int32, device=dev)
            part = torch.zeros(T.query("tnr_grad_sumsq_parts", eng.n_train), dtype=torch.float32, device=dev)
            g, n = eng.flat_g, eng.n_train
            scans = {"tnr_grad_nonfinite_scan": lambda: T.call("tnr_grad_nonfinite_scan", g, n, guard, 1),
                     "tnr_grad_sumsq_scan_guard": lambda: T.call("tnr_grad_sumsq_scan", g, n, part, guard, 1),
                     "tnr_grad_sumsq_scan": lambda: T.call("tnr_grad_sumsq_scan", g, n, part, None, 0)}
            su = {k: [] for k in scans}
            for fn in scans.values():
                timed(fn, 5)
            for _ in range(a.rounds):
                for k, fn in scans.items():
                    su[k] += timed(fn, a.steps)
            y = {k: stats(v) for k, v in su.items()}
            for k in y:
                y[k]["GB_per_s"] = round(4.0 * n / (1e3 * y[k]["median_us"]), 1)
            base = y["tnr_grad_nonfinite_scan"]
            y["fused_over_plain"] = round(y["tnr_grad_sumsq_scan_guard"]["median_us"] / base["median_us"], 3)
            y["plain_spread_p90_over_p10"] = round(base["p90_us"] / base["p10_us"], 3)
            out["scan_whole_gradient"] = y
        del eng
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
