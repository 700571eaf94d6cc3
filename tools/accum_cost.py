"""What --grad_accum_steps costs, on one GPU at bench.py's headline shape (4 layers, (2, 3) trainable, 4 teachers, B = 32).

part "kernel": tnr_grad_accum alone at the headline's n_train, in its three uses - first micro-batch (acc <- g, overwrite: 8 bytes
per element), the ones between (acc += g: 12) and the last (g += acc: 12) - and, in the same run, tnr_grad_nonfinite_scan over the
same buffer as the read-only yardstick (4 bytes per element, the kernel whose memory shape this one follows).  Each launch between
two events; the variants alternate in rounds; median, 10th / 90th percentile and the achieved bytes per second.  Both buffers
together (119 MB) fit the 256 MB last-level cache, as they do in training, where the backward in front has just written flat_g.

part "window": forward + backward(micro=(j, K)) for j < K, then ONE step(grad_scale = 1 / K), against K times forward + backward +
step of the path without accumulation, K = 2 and 4, fp16; bracketed from the first forward to the end of the last step, the two
alternating.  The window makes K - 1 optimiser steps FEWER and K accumulation passes more.

The parts run one behind the other as child processes, each under a time limit of its own; the second starts only if the first
ended well.  EXPERIMENTS.md item 68 records the output.

    python tools/accum_cost.py [--rounds 6] [--steps 40] [--batch 32]      -> one JSON line per part"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tiny-newsrec_amd"))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np   # noqa: E402
import torch         # noqa: E402

from adamw_cost import stats, timed   # noqa: E402

LIMIT = {"kernel": 240, "window": 420}       # seconds


def headline_engine(batch, dtype="fp16"):
    import engine as E
    import hashinit
    from schema import FULL, state_shapes
    torch.cuda.set_device(0)
    cfg = E.EngineConfig()
    eng = E.Engine(cfg, "cuda:0", max_batch=batch, dtype=dtype)
    eng.load_state_dict(hashinit.init_state_dict(1234, state_shapes(FULL, cfg.n_layers, cfg.D, cfg.T)))
    return eng


def part_kernel(a):
    import tnr_hip as T
    eng = headline_engine(a.batch)
    n, dev = eng.n_train, "cuda:0"
    g = eng.flat_g
    g.copy_(torch.randn(n, device=dev, generator=torch.Generator(device=dev).manual_seed(5)) * 1e-3)
    acc = eng._acc_buffer()
    guard = torch.zeros(4, dtype=torch.int32, device=dev)
    uses = {"first (acc <- g)": (lambda: T.call("tnr_grad_accum", acc, g, n, 1), 8),
            "middle (acc += g)": (lambda: T.call("tnr_grad_accum", acc, g, n, 0), 12),
            "last (g += acc)": (lambda: T.call("tnr_grad_accum", g, acc, n, 0), 12),
            "yardstick: tnr_grad_nonfinite_scan(g)": (lambda: T.call("tnr_grad_nonfinite_scan", g, n, guard, 1), 4)}
    us = {k: [] for k in uses}
    for k, (fn, _) in uses.items():
        timed(fn, 5)
    for _ in range(a.rounds):
        for k, (fn, _) in uses.items():
            acc.zero_()                      # "last" doubles g every launch otherwise: keep the values finite and small
            us[k] += timed(fn, a.steps)
    out = {"n_train": int(n), "buffer_MB": round(4e-6 * n, 1)}
    for k, (_, b) in uses.items():
        s = stats(us[k])
        s["bytes_per_element"], s["derived_MB"] = b, round(1e-6 * b * n, 1)
        s["TB_per_s"] = round(b * n / s["median_us"] * 1e-6, 2)
        out[k] = s
    return out


def part_window(a):
    import synth
    eng = headline_engine(a.batch)
    cfg, dev, B = eng.cfg, "cuda:0", a.batch
    d = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    n_news = 20000
    comb, tabs = d(synth.news_table(7, n_news, cfg.L)), d(synth.teacher_tables(7, cfg.T, n_news, cfg.D))
    hidx, mask, cidx, label = [d(x) for x in synth.impressions(8, 4 * B, n_news, cfg.U, cfg.C)]

    def fwd(j):
        s = slice(j * B, (j + 1) * B)
        eng.forward_indexed(comb, hidx[s], mask[s], cidx[s], label[s], tabs)

    def plain(K):
        for j in range(K):
            fwd(j)
            eng.backward()
            eng.step(1e-6)

    def window(K):
        for j in range(K):
            fwd(j)
            eng.backward(micro=(j, K))
        eng.step(1e-6, grad_scale=1.0 / K)
    out = {"batch": B, "dtype": "fp16"}
    reps = max(a.steps // 4, 5)
    for K in (2, 4):
        us = {"plain": [], "window": []}
        timed(lambda: plain(K), 3), timed(lambda: window(K), 3)
        for _ in range(a.rounds):
            us["plain"] += timed(lambda: plain(K), reps)
            us["window"] += timed(lambda: window(K), reps)
        s = {k: stats(v) for k, v in us.items()}
        s["window_minus_plain_us"] = round(s["window"]["median_us"] - s["plain"]["median_us"], 1)
        s["ratio"] = round(s["window"]["median_us"] / s["plain"]["median_us"], 4)
        out["K=%d" % K] = s
    eng.scaler.drain(eng)
    out["skipped_steps"] = int(eng.scaler.skipped)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--steps", type=int, default=40, help="launches per use and round (windows: a quarter of it)")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--part", default=None, choices=sorted(LIMIT), help=argparse.SUPPRESS)     # the child of one part
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/accum_cost.py measures on the GPU: none found")
    if a.part:
        print(json.dumps({a.part: (part_kernel if a.part == "kernel" else part_window)(a)}))
        return
    for part in ("kernel", "window"):        # chained: a part that fails or runs out of time ends the run
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--rounds", str(a.rounds), "--steps", str(a.steps), "--batch",
                            str(a.batch), "--part", part], capture_output=True, text=True, timeout=LIMIT[part])
        if r.returncode != 0:
            raise SystemExit("part %s failed (%d):\n%s" % (part, r.returncode, (r.stdout + r.stderr)[-2000:]))
        print(r.stdout.strip().splitlines()[-1], flush=True)


if __name__ == "__main__":
    main()
