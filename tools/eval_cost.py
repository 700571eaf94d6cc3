"""What the impression loop of test mode costs on the host (the reference's loop, run.test's default) and on the device
(--device_metrics True: one Engine.evaluate per batch), in impressions per second, and what the rank-metrics kernel
(tnr_rank_metrics, csrc/evaluate.hip) costs alone.  The yardstick is the host loop on the same inputs in the same process:
the feature has no earlier version to compare with.

Inputs: a synthetic table of 51 200 news x 256 (standard normal, as if encoded - news encoding is not part of either loop),
hash-initialised user-encoder weights, and MIND-shaped impressions: histories of 1 .. 50 clicks, candidate counts from a
fixed-seed log-normal clipped to 2 .. 300 (mean about 37), one to three positives each.  Both loops are run.py's own
(_impression_loop) over the same pre-decoded batches, so the file decode is in neither; each is timed wall-clock around the
whole loop, its final read-back included, `--rounds` times alternating, median reported.  The kernel alone is timed with HIP
events over one launch of `--kernel_batch` impressions (scores, per-impression values and totals) on operands that are already
on the device, beside its DERIVED floor: the gathered bytes (candidates x D x 4) at the HBM rate (8 TB/s).  EXPERIMENTS.md
records the output.

    python tools/eval_cost.py [--impressions 4096] [--batch_sizes 32 128 256] [--rounds 3] [--kernel_batch 4096]   -> one JSON line"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tiny-newsrec_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import numpy as np   # noqa: E402
import torch         # noqa: E402

HBM_BYTES_PER_S = 8.0e12
N_NEWS, D, U = 51200, 256, 50


def impressions(n, seed=7):
    """-> hist (n, U) int32, mask (n, U) f32, [cand arrays], [label arrays]"""
    rng = np.random.default_rng(seed)
    sizes = np.clip(np.round(rng.lognormal(3.25, 0.85, n)), 2, 300).astype(np.int64)
    hist = rng.integers(1, N_NEWS, size=(n, U)).astype(np.int32)
    clicks = rng.integers(1, U + 1, size=n)
    mask = (np.arange(U)[None, :] >= U - clicks[:, None]).astype(np.float32)        # front-padded, as pad_to_fix_len pads
    hist *= mask.astype(np.int32)
    cands, labels = [], []
    for c in sizes:
        cands.append(rng.integers(1, N_NEWS, size=c))
        y = np.zeros(c, np.int64)
        y[rng.permutation(c)[:min(int(rng.integers(1, 4)), c - 1)]] = 1
        labels.append(y)
    return hist, mask, cands, labels


class Batches:
    """What DataLoaderTest yields, decoded beforehand: (hist_idx, mask on the device, [cands], [labels]) per batch."""

    def __init__(self, hist, mask, cands, labels, B, dev):
        self.items = [(torch.from_numpy(hist[i:i + B]).to(dev), torch.from_numpy(mask[i:i + B]).to(dev), cands[i:i + B], labels[i:i + B])
                      for i in range(0, len(cands), B)]

    def __iter__(self):
        return iter(self.items)

    def join(self):
        pass


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--impressions", type=int, default=4096)
    ap.add_argument("--batch_sizes", type=int, nargs="+", default=[32, 128, 256])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--kernel_batch", type=int, default=4096)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/eval_cost.py measures on the GPU: none found")
    import engine as E
    import hashinit
    import run
    import tnr_hip as T
    from helpers import FULL, state_shapes
    dev = "cuda:0"
    torch.cuda.set_device(0)
    gen = torch.Generator(device=dev).manual_seed(11)
    news = torch.randn((N_NEWS, D), device=dev, generator=gen)
    hist, mask, cands, labels = impressions(a.impressions)
    n_cand = int(sum(len(c) for c in cands))
    out = {"news": N_NEWS, "D": D, "impressions": a.impressions, "candidates": n_cand, "mean_candidates": round(n_cand / a.impressions, 1),
           "max_candidates": int(max(len(c) for c in cands)), "rounds": a.rounds, "hbm_bytes_per_s": HBM_BYTES_PER_S, "loops": {}}
    P = hashinit.init_state_dict(7, state_shapes(FULL, 1, D, 0))
    for B in a.batch_sizes:
        eng = E.Engine(E.EngineConfig(n_layers=1, trainable_layers=(), num_teachers=0, news_dim=D, user_log_length=U), dev, max_batch=B)
        eng.load_state_dict(P)
        batches = Batches(hist, mask, cands, labels, B, dev)
        res, secs = {}, {"host": [], "device": []}
        for r in range(a.rounds + 1):                                        # round 0 warms both up
            for name in ("host", "device"):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                res[name] = run._impression_loop(eng, news, batches, 0, 10 ** 9, device_metrics=name == "device")
                torch.cuda.synchronize()
                if r:
                    secs[name].append(time.perf_counter() - t0)
        (hs, hn, hm), (ds, dn, dm) = res["host"], res["device"]
        assert hn == dn == a.impressions and hm == dm
        med = {k: float(np.median(v)) for k, v in secs.items()}
        out["loops"][str(B)] = {
            "host_impressions_per_s": round(a.impressions / med["host"], 1), "device_impressions_per_s": round(a.impressions / med["device"], 1),
            "host_s": round(med["host"], 4), "device_s": round(med["device"], 4), "device_over_host": round(med["host"] / med["device"], 2),
            "scored": hm, "mean_metrics_host": [round(float(x) / hm, 5) for x in hs], "mean_metrics_device": [round(float(x) / dm, 5) for x in ds]}
        del eng
        torch.cuda.empty_cache()
    # the kernel alone
    KB = min(a.kernel_batch, a.impressions)
    c, y, o = E.pack_impressions(cands[:KB], labels[:KB])
    users = torch.randn((KB, D), device=dev, generator=gen)
    ct, yt, ot = (torch.from_numpy(x).to(dev) for x in (c, y, o))
    scores = torch.empty((c.size,), device=dev, dtype=torch.float32)
    per = torch.empty((KB, 4), device=dev, dtype=torch.float64)
    acc = torch.empty((6,), device=dev, dtype=torch.float64)
    fn = lambda: T.call("tnr_rank_metrics", users, D, KB, news, D, N_NEWS, D, ot, ct, yt, scores, per, acc, 0)
    for _ in range(3):
        fn()
    ev = []
    for _ in range(20):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        ev.append((e0, e1))
    torch.cuda.synchronize()
    us = np.array([1e3 * p.elapsed_time(q) for p, q in ev])
    floor = 1e6 * c.size * D * 4 / HBM_BYTES_PER_S
    out["kernel"] = {"impressions": KB, "candidates": int(c.size), "median_us": round(float(np.median(us)), 1),
                     "p10_us": round(float(np.percentile(us, 10)), 1), "p90_us": round(float(np.percentile(us, 90)), 1),
                     "gathered_bytes": int(c.size) * D * 4, "hbm_floor_us": round(floor, 1),
                     "floor_reached": round(floor / float(np.median(us)), 3),
                     "impressions_per_s": round(KB / (float(np.median(us)) * 1e-6), 0)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
