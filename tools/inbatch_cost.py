"""What --inbatch_negatives costs: the device time of forward + backward with the option off and on, on one GPU at bench.py's
headline model (4 layers, (2, 3) trainable, 4 teachers, U = 50, C = 5, L = 30, D = 256, fp16), at B = 32 and B = 128, fed by index
from resident tables with synth.impressions' batches (no de-duplication plan: the option's own work does not depend on one).

Every forward + backward is bracketed with a pair of events, so a figure is the time from the step's first kernel to the end of the
backward, launch gaps included.  The two legs alternate in rounds within one process; each reports median and the 10th / 90th
percentile over all its steps: compare the difference against that spread.  With the option off Engine.forward and backward make the
calls of the commit before the option existed, in the same order (tests/test_inbatch_gpu.py::test_off_is_the_step_as_it_was), so
the off leg IS that commit's step; on a tree without the option the script times the off leg alone, for a run of both trees.
Then a few more steps run with every C-ABI call bracketed (tnr_hip.TIMED_ALL) and the three new entry points are reported one by
one: tnr_inbatch_plan is two launches, tnr_inbatch_loss two, tnr_inbatch_bwd one.

The derived expectation at B = 32: 32 x 160 logits of 256 fma and as much again in the backward, under 1 MB of traffic - the cost of
the five launches.  EXPERIMENTS.md records the output.

    python tools/inbatch_cost.py [--rounds 6] [--steps 20] [--batches 32 128]      -> one JSON line"""
import argparse
import inspect
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


def measure(a, B):
    import engine as E
    import hashinit
    import synth
    import tnr_hip as T
    from schema import FULL, state_shapes
    dev = "cuda:0"
    torch.cuda.set_device(0)
    cfg = E.EngineConfig()
    has = "inbatch" in inspect.signature(E.Engine.forward_indexed).parameters
    eng = E.Engine(cfg, dev, max_batch=B, dtype=a.dtype)
    eng.load_state_dict(hashinit.init_state_dict(1234, state_shapes(FULL, cfg.n_layers, cfg.D, cfg.T)))
    n_news, n_feeds = 4000, 4
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    comb = t(synth.news_table(5, n_news, cfg.L))
    tabs = t(synth.teacher_tables(5, cfg.T, n_news, cfg.D).astype(np.float32))
    h, m, c, y = [t(x) for x in synth.impressions(77, n_feeds * B, n_news, cfg.U, cfg.C)]
    feeds = [(h[i * B:(i + 1) * B].contiguous(), m[i * B:(i + 1) * B].contiguous(), c[i * B:(i + 1) * B].contiguous(),
              y[i * B:(i + 1) * B].contiguous()) for i in range(n_feeds)]
    k = [0]

    def step(on):
        hh, mm, cc, yy = feeds[k[0] % n_feeds]
        k[0] += 1
        eng.forward_indexed(comb, hh, mm, cc, yy, tabs, **(dict(inbatch=True) if on else {}))
        eng.backward()
    legs = {"off": False, "on": True} if has else {"off": False}
    us = {n: [] for n in legs}
    for n, on in legs.items():
        timed(lambda: step(on), 5)
    for _ in range(a.rounds):
        for n, on in legs.items():
            us[n] += timed(lambda: step(on), a.steps)
    r = {n: stats(v) for n, v in us.items()}
    if has:
        r["on minus off"] = {"extra_us": round(r["on"]["median_us"] - r["off"]["median_us"], 1),
                             "ratio": round(r["on"]["median_us"] / r["off"]["median_us"], 4),
                             "off_p10_p90_spread_us": round(r["off"]["p90_us"] - r["off"]["p10_us"], 1)}
        r["eligible_per_impression"] = round(float(eng.inbatch_counts().float().mean()), 1)
        T.TIMED_ALL = []
        for _ in range(a.steps):
            step(True)
        torch.cuda.synchronize()
        per = {}
        for e0, e1, name in T.TIMED_ALL:
            if name.startswith("tnr_inbatch"):
                per.setdefault(name, []).append(1e3 * e0.elapsed_time(e1))
        T.TIMED_ALL = None
        r["calls"] = {n: stats(v) for n, v in per.items()}
    del eng
    torch.cuda.empty_cache()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--steps", type=int, default=20, help="steps per leg and round")
    ap.add_argument("--batches", type=int, nargs="+", default=[32, 128])
    ap.add_argument("--dtype", default="fp16")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/inbatch_cost.py measures on the GPU: none found")
    print(json.dumps({"dtype": a.dtype, "rounds": a.rounds, "steps_per_round": a.steps,
                      "forward_backward": {"B%d" % B: measure(a, B) for B in a.batches}}))


if __name__ == "__main__":
    main()
