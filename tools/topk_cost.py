"""What the fused score-and-select call (tnr_topk_scores, csrc/retrieve.hip) costs beside a plain tnr_sgemm that materialises the
same Nu x Nn scores and selects nothing - the yardstick, since the feature has no earlier version to compare with.

Both are timed with HIP events in ONE process, alternating in rounds, on the same standard-normal operands; each reports
median and the 10th / 90th percentile over all its calls.  Shapes: 32 x 51 200 x 256 with K = 10 (online: one user tile, the
news table cut into parts) and 4 096 x 51 200 x 256 with K = 100 (offline; 840 MB of scores, which the yardstick still fits).
--big 1 also times the fused call alone, three calls after one warm-up, at 65 536 x 130 000 x 256 with K = 100 (34 GB of scores
that are never written).  Beside the times: the ratio fused / sgemm and the fraction reached of the two DERIVED floors -
2 Nu Nn D FLOP at the fp32 matrix peak (157 TFLOP/s) and one pass over the Nn D 4-byte news table per user tile at the rate the
last-level cache serves a table of that size (8.6 TB/s, the chip's measured figure for a 38 MB table).  EXPERIMENTS.md item 72
records the output.

    python tools/topk_cost.py [--rounds 5] [--calls 10] [--big 0]      -> one JSON line"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tiny-newsrec_amd"))
sys.path.insert(0, ROOT)

import numpy as np   # noqa: E402
import torch         # noqa: E402

PEAK_FLOPS, LLC_BYTES_PER_S = 157e12, 8.6e12


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


def fused_call(T, users, news, K, splits=0):
    Nu, D = users.shape
    Nn = news.shape[0]
    idx = torch.empty((Nu, K), dtype=torch.int32, device=users.device)
    sc = torch.empty((Nu, K), dtype=torch.float32, device=users.device)
    nb = int(T.query("tnr_topk_workspace", Nu, Nn, K, splits))
    work = torch.empty((max(nb, 8),), dtype=torch.uint8, device=users.device)
    return (lambda: T.call("tnr_topk_scores", users, D, Nu, news, D, Nn, 1, D, None, 0, 0, K, idx, sc, splits, work, nb)), nb


def floors(Nu, Nn, D, K):
    users_per_tile = 32 * min(4, -(-Nu // 32), (160 * 1024 - 33792) // (K * 256 + 3072))      # csrc/retrieve.hip: tk_waves
    tiles = -(-Nu // users_per_tile)
    return {"flop_floor_us": round(2e6 * Nu * Nn * D / PEAK_FLOPS, 1), "news_pass_floor_us": round(1e6 * tiles * Nn * D * 4 / LLC_BYTES_PER_S, 1),
            "user_tiles": tiles}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10, help="calls per variant and round")
    ap.add_argument("--big", type=int, default=0)
    a = ap.parse_args()
    import tnr_hip as T
    if not torch.cuda.is_available():
        raise SystemExit("tools/topk_cost.py measures on the GPU: none found")
    dev = "cuda:0"
    torch.cuda.set_device(0)
    gen = torch.Generator(device=dev).manual_seed(11)
    out = {"rounds": a.rounds, "calls_per_round": a.calls, "peak_flops": PEAK_FLOPS, "llc_bytes_per_s": LLC_BYTES_PER_S, "shapes": {}}
    for name, Nu, Nn, D, K in (("online", 32, 51200, 256, 10), ("offline", 4096, 51200, 256, 100)):
        users = torch.randn((Nu, D), device=dev, generator=gen)
        news = torch.randn((Nn, D), device=dev, generator=gen)
        scores = torch.empty((Nu, Nn), device=dev, dtype=torch.float32)
        fused, nb = fused_call(T, users, news, K)
        sgemm = lambda: T.call("tnr_sgemm", users, D, 1, 0, None, news, D, 1, 0, scores, Nn, 0, None, 0, Nu, Nn, D, 1, 1.0, 0.0, 1, None)
        variants = {"fused": fused, "sgemm": sgemm}
        calls = a.calls if name == "online" else max(2, a.calls // 3)
        us = {k: [] for k in variants}
        for fn in variants.values():
            timed(fn, 2)
        for _ in range(a.rounds):
            for k, fn in variants.items():
                us[k] += timed(fn, calls)
        r = {k: stats(v) for k, v in us.items()}
        r.update(floors(Nu, Nn, D, K))
        r["Nu"], r["Nn"], r["D"], r["K"], r["workspace_bytes"] = Nu, Nn, D, K, nb
        r["fused_over_sgemm"] = round(r["fused"]["median_us"] / r["sgemm"]["median_us"], 3)
        r["sgemm_spread_p90_over_p10"] = round(r["sgemm"]["p90_us"] / r["sgemm"]["p10_us"], 3)
        for k in ("fused", "sgemm"):
            r[k]["TFLOPs"] = round(2e-6 * Nu * Nn * D / r[k]["median_us"], 2)
        r["flop_floor_reached"] = round(r["flop_floor_us"] / r["fused"]["median_us"], 3)
        r["news_pass_floor_reached"] = round(r["news_pass_floor_us"] / r["fused"]["median_us"], 3)
        out["shapes"][name] = r
        del users, news, scores
        torch.cuda.empty_cache()
    if a.big:
        Nu, Nn, D, K = 65536, 130000, 256, 100
        users = torch.randn((Nu, D), device=dev, generator=gen)
        news = torch.randn((Nn, D), device=dev, generator=gen)
        fused, nb = fused_call(T, users, news, K)
        timed(fused, 1)
        ts = timed(fused, 3)
        t = float(np.median(ts))
        r = {"fused_us": round(t, 1), "all_us": [round(x, 1) for x in ts], "n": 3, "Nu": Nu, "Nn": Nn, "D": D, "K": K, "workspace_bytes": nb, "TFLOPs": round(2e-6 * Nu * Nn * D / t, 2)}
        r.update(floors(Nu, Nn, D, K))
        r["flop_floor_reached"] = round(r["flop_floor_us"] / t, 3)
        r["news_pass_floor_reached"] = round(r["news_pass_floor_us"] / t, 3)
        out["shapes"]["big_fused_alone"] = r
    print(json.dumps(out))


if __name__ == "__main__":
    main()
