"""What --save_optimizer costs at an epoch end, on one GPU at bench.py's headline shape (4 layers, (2, 3) trainable, 4 teachers).

The engine takes a few optimiser steps on a random flat_g with everything on (so the moments, vmax and the average hold values),
then run.py's checkpoint dict is built and written twice to a temporary directory, without and with the optimiser state:
wall time of optimizer_state_dict() (device-to-host copies of the three moment buffers, slot by slot), of torch.save of each dict,
and the two file sizes; the derived size 12 bytes per trainable element beside them.  Recorded values, not bounds: nothing here is
on the step's path.  EXPERIMENTS.md item 70 records the output.

    python tools/ckpt_cost.py [--reps 3] [--dir DIR]      -> one JSON line"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tiny-newsrec_amd"))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch         # noqa: E402

from accum_cost import headline_engine   # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--dir", default=None, help="where the checkpoints are written (default: a temporary directory)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/ckpt_cost.py measures on the GPU: none found")
    eng = headline_engine(32)
    g = torch.Generator(device="cuda:0").manual_seed(5)
    for _ in range(3):
        eng.flat_g.copy_(torch.randn(eng.n_train, device="cuda:0", generator=g) * 1e-3)
        eng.step(1e-4, weight_decay=0.01, warmup_steps=2, ema_decay=0.9, max_grad_norm=1.0)
    torch.cuda.synchronize()
    n_slots = sum(v[2] for v in eng.slot.values() if v[0])
    out = {"n_train": int(eng.n_train), "trainable_elements": int(n_slots), "derived_MB": round(12e-6 * n_slots, 1),
           "optimizer_state_dict_ms": [], "save_without_ms": [], "save_with_ms": []}
    with tempfile.TemporaryDirectory(dir=a.dir) as d:
        for _ in range(a.reps):
            ckpt = {"model_state_dict": {k: v.cpu() for k, v in eng.state_dict().items()}, "category_dict": {}, "word_dict": None,
                    "subcategory_dict": {}, "ema_state_dict": {k: v.cpu() for k, v in eng.ema_state_dict().items()}}
            t0 = time.perf_counter()
            torch.save(ckpt, os.path.join(d, "without.pt"))
            t1 = time.perf_counter()
            osd = eng.optimizer_state_dict()
            t2 = time.perf_counter()
            ckpt["optimizer_state_dict"] = osd
            ckpt["train_state"] = {"epoch": 1, "updates": eng.step_count, "flags": {}}
            torch.save(ckpt, os.path.join(d, "with.pt"))
            t3 = time.perf_counter()
            out["save_without_ms"].append(round(1e3 * (t1 - t0), 1))
            out["optimizer_state_dict_ms"].append(round(1e3 * (t2 - t1), 1))
            out["save_with_ms"].append(round(1e3 * (t3 - t2), 1))
        out["file_without_MB"] = round(1e-6 * os.path.getsize(os.path.join(d, "without.pt")), 1)
        out["file_with_MB"] = round(1e-6 * os.path.getsize(os.path.join(d, "with.pt")), 1)
    out["added_MB"] = round(out["file_with_MB"] - out["file_without_MB"], 1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
