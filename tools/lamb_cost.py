"""What --optimizer lamb costs: the device time of Engine.step with LAMB off and on, fp16 / AMSGrad and bf16 / Adam, on one GPU at
bench.py's headline shape (4 layers, (2, 3) trainable, 4 teachers, B = 32: 14.9 M trainable elements).

flat_g is filled once with N(0, 1e-3^2) (no forward: the optimiser step does not care where its gradient came from); every
Engine.step is bracketed with a pair of events, as bench.py's step_breakdown_ms brackets its calls, so a figure is the time from the
step's first kernel to the end of the weight-copy refresh, launch gaps included.  The two legs alternate in rounds within one
process, and each reports median and the 10th / 90th percentile over all its steps: compare differences against that spread.  With
LAMB off, Engine.step makes the calls of the parent commit in the same order, so the off leg IS the parent's step.

The derived expectation: the update moves 36 n bytes with AMSGrad (5 reads, 4 writes of 4 bytes) and 28 n with plain Adam; the norm
pass reads p, g, m, v (and vmax) again and writes nothing per element: + 20 n / + 16 n bytes, 1.56x / 1.57x the bytes of the update
(the commit reads 8 bytes per 4096 elements; the step's other kernels - the fp16 scan, the weight-copy refresh - do not grow; a
tensor that is not adapted is not read by the norm pass, 0.4 % of the elements here).  The caveat of EXPERIMENTS.md item 67 applies:
the loop that is timed touches 5 (AMSGrad) or 4 buffers of 4 n bytes = 298 / 238 MB at the headline's n, around the size of the
256 MB last-level cache, so part of what the norm pass re-reads, and of what the next step reads, can come from the cache in this
loop and would come from HBM behind a real forward / backward; the figure is a lower bound of the cost in training.
EXPERIMENTS.md item 76 records the output.

    python tools/lamb_cost.py [--rounds 6] [--steps 40] [--batch 32]      -> one JSON line"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tiny-newsrec_amd"))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np   # noqa: E402
import torch         # noqa: E402

from adamw_cost import stats, timed   # noqa: E402


def measure(a):
    import engine as E
    import hashinit
    from schema import FULL, state_shapes
    dev, seed = "cuda:0", 1234
    torch.cuda.set_device(0)
    cfg = E.EngineConfig()
    sd = hashinit.init_state_dict(seed, state_shapes(FULL, cfg.n_layers, cfg.D, cfg.T))
    out = {}
    for dtype, ams in (("fp16", True), ("bf16", False)):
        eng = E.Engine(cfg, dev, max_batch=a.batch, dtype=dtype)
        eng.load_state_dict(sd)
        eng.flat_g.copy_(torch.randn(eng.n_train, device=dev, generator=torch.Generator(device=dev).manual_seed(5)) * 1e-3)
        pos = 0
        for s_, e_ in sorted(eng.bucket_ranges()) + [(eng.n_train, eng.n_train)]:       # alignment gaps hold zeros after a backward
            eng.flat_g[pos:s_].zero_()
            pos = max(pos, e_)
        norm = 1e-3 * float(np.sqrt(eng.n_train))
        full = {"warmup_steps": 1000000, "lr_decay_steps": 2000000, "weight_decay": 0.01, "max_grad_norm": 0.5 * norm}
        variants = {"off": {"amsgrad": ams}, "lamb": {"amsgrad": ams, "lamb": True},
                    "decay_schedule_clip": dict(full, amsgrad=ams), "lamb_decay_schedule_clip": dict(full, amsgrad=ams, lamb=True)}
        us = {k: [] for k in variants}
        for k, kw in variants.items():                                              # warm-up: every variant's kernels and buffers
            timed(lambda: eng.step(1e-4, **kw), 5)
        for _ in range(a.rounds):
            for k, kw in variants.items():
                us[k] += timed(lambda: eng.step(1e-4, **kw), a.steps)
        r = {k: stats(v) for k, v in us.items()}
        b, extra = (36, 20) if ams else (28, 16)
        ls = eng._lamb_state
        r.update(n_train=int(eng.n_train), gradient_MB=round(4e-6 * eng.n_train, 1), update="amsgrad" if ams else "adam",
                 chunks=int(ls.n_chunks), tensors=int(ls.n_tensors), adapted_tensors=len(ls.adapted),
                 buffers_touched_MB=round(4e-6 * eng.n_train * (b // 8 + 1)), derived_update_bytes_ratio=round((b + extra) / b, 4))
        cmp_ = {}
        for k, base in (("lamb", "off"), ("lamb_decay_schedule_clip", "decay_schedule_clip")):
            cmp_["%s over %s" % (k, base)] = {"ratio": round(r[k]["median_us"] / r[base]["median_us"], 4),
                                             "extra_us": round(r[k]["median_us"] - r[base]["median_us"], 1),
                                             "base_p10_p90_spread_us": round(r[base]["p90_us"] - r[base]["p10_us"], 1)}
        r["compare"] = cmp_
        tr = eng.trust_ratios()
        ts = sorted(t for t, _, _ in tr.values())
        r["trust_min_median_max"] = [ts[0], ts[len(ts) // 2], ts[-1]]
        out[dtype] = r
        del eng
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--steps", type=int, default=40, help="steps per variant and round")
    ap.add_argument("--batch", type=int, default=32)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/lamb_cost.py measures on the GPU: none found")
    print(json.dumps({"batch": a.batch, "rounds": a.rounds, "steps_per_round": a.steps, "step": measure(a)}))


if __name__ == "__main__":
    main()
