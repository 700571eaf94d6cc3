"""Stage 1 in train mode: interleaved same-process A/B of the whole step (forward_indexed + backward + plain two-rate Adam, as
bench.py's stage-1 legs run it) at both bench shapes - 30 / 128 with 1 + 4 titles and 24 / 512 with 1 + 9 titles, B = 32, 2-layer
student training both layers, 4 teachers, fp16 - in three modes:
    per_pass_drop   Stage1Engine.joint = False, dropout 0.1 / 0.1 (what every train-mode run took before the split sites)
    joint_drop      the joint passes, dropout 0.1 / 0.1 (the train-mode default now)
    joint_eval      the joint passes, dropout off (bench.py's stage-1 legs)
GPU box:  python tools/s1_train_mode.py [--rounds 6] [--steps 20] [--shape 30/128] [--json out.json]
Launch counts:  rocprofv3 --kernel-trace --stats -d DIR -- python tools/s1_train_mode.py --launches
runs one step of each mode between two marker launches of scale_inplace_kernel (a kernel no step launches) and prints the C
entry-point calls of that step (tnr_hip.TIMED_ALL); python tools/s1_train_mode.py --count DIR/.../*_results.db (or a kernel_trace.csv) then counts
the kernels between each pair of markers in the trace (in dispatch order)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tiny-newsrec_amd"))
import numpy as np      # noqa: E402
import torch            # noqa: E402

import hashinit         # noqa: E402
import synth            # noqa: E402
import tnr_hip as T     # noqa: E402
from stage1 import Stage1Engine   # noqa: E402

SHAPES = {"30/128": (30, 128, 4), "24/512": (24, 512, 9)}
MODES = ("per_pass_drop", "joint_drop", "joint_eval")
B, ND, SEED = 32, 20000, 1234


def setup(Lt, Lb, Kn, n_batches, dev="cuda:0"):
    s1 = Stage1Engine(n_layers=2, trainable_layers=(0, 1), num_teachers=4, npratio=Kn, title_len=Lt, body_len=Lb, device=dev, batch=B,
                      dtype="fp16")
    s1.load_state_dict({k: torch.from_numpy(hashinit.init_tensor(SEED, k, tuple(sh))) for k, sh in s1.shapes.items()})
    s1.title.refresh_shadows(all_layers=True)
    s1.body.refresh_rel()
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    data = dict(title=t(synth.news_table(11, ND - 1, Lt)), body=t(synth.news_table(12, ND - 1, Lb, mean_len=0.6 * Lb, std_len=0.25 * Lb)),
                tt=t(synth.teacher_tables(13, 4, ND - 1, s1.cfg_t.D)), tb=t(synth.teacher_tables(14, 4, ND - 1, s1.cfg_t.D)))
    pidx = t(np.random.RandomState(SEED).randint(1, ND, (n_batches * B, 1 + Kn)).astype(np.int32))
    data.update(pidx=pidx, pcol=pidx[:, 0].contiguous(), label=torch.zeros(B, dtype=torch.int64, device=dev))
    return s1, data


def set_mode(s1, mode):
    s1.joint = mode != "per_pass_drop"
    if mode == "joint_eval":
        s1.set_dropout(0.0, 0.0, SEED)
    else:
        s1.set_dropout(0.1, 0.1, SEED)


def step(s1, d, i):
    s = slice(i * B, (i + 1) * B)
    s1.forward_indexed(d["title"], d["body"], d["pidx"][s], d["label"], d["tt"], d["tb"], body_idx=d["pcol"][s])
    s1.backward()
    s1.step(1e-5, lr_bert=1e-6, amsgrad=False)


def count_kernels(path):
    """path: the kernel_trace.csv of rocprofv3's csv output, or the SQLite database of its default output (`kernels` view)."""
    if path.endswith(".db"):
        import sqlite3
        names = [r[0] for r in sqlite3.connect(path).execute("SELECT name FROM kernels ORDER BY dispatch_id")]
    else:
        import csv
        with open(path) as f:
            rows = list(csv.DictReader(f))
        key = "Correlation_Id" if "Correlation_Id" in rows[0] else "Dispatch_Id"
        names = [r["Kernel_Name"] for r in sorted(rows, key=lambda r: int(r[key]))]
    inside, n, spans = False, 0, []
    for name in names:
        if "scale_inplace_kernel" in name:
            if inside:
                spans.append(n)
            inside, n = not inside, 0
        elif inside:
            n += 1
    print("kernels per marked step, in --launches order (per shape: %s):" % ", ".join(MODES), spans)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shape", choices=list(SHAPES), action="append")
    ap.add_argument("--launches", action="store_true", help="one step per mode with the C entry points counted (for a kernel trace)")
    ap.add_argument("--count", default=None, help="rocprofv3 output (.db or kernel_trace.csv) of a --launches run: kernels per marked step")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if a.count:
        count_kernels(a.count)
        return
    out = {}
    for key in (a.shape or list(SHAPES)):
        Lt, Lb, Kn = SHAPES[key]
        s1, d = setup(Lt, Lb, Kn, a.warmup + a.steps)
        if a.launches:
            marker = torch.zeros(1, device="cuda:0")
            for mode in MODES:
                set_mode(s1, mode)
                for i in range(a.warmup):
                    step(s1, d, i)
                torch.cuda.synchronize()
                print("=== begin %s %s" % (key, mode), flush=True)
                T.call("tnr_scale_inplace", marker, 1, 1.0)
                T.TIMED_ALL = []
                step(s1, d, 0)
                calls = T.TIMED_ALL
                T.TIMED_ALL = None
                T.call("tnr_scale_inplace", marker, 1, 1.0)
                torch.cuda.synchronize()
                print("=== end %s %s: %d entry-point calls, joint %s" % (key, mode, len(calls), s1.ran_joint), flush=True)
                out.setdefault(key, {})[mode] = {"entry_point_calls": len(calls), "ran_joint": bool(s1.ran_joint)}
            continue
        res = {m: [] for m in MODES}
        for r in range(a.rounds):
            order = MODES if r % 2 == 0 else MODES[::-1]          # interleaved: drifts of clock / temperature hit every mode alike
            for mode in order:
                set_mode(s1, mode)
                for i in range(a.warmup):
                    step(s1, d, i)
                assert s1.ran_joint == (mode != "per_pass_drop")
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for i in range(a.warmup, a.warmup + a.steps):
                    step(s1, d, i)
                torch.cuda.synchronize()
                res[mode].append((time.perf_counter() - t0) / a.steps * 1e3)
        med = {m: float(np.median(v)) for m, v in res.items()}
        out[key] = {m: {"median_ms": round(med[m], 4), "min_ms": round(min(res[m]), 4), "max_ms": round(max(res[m]), 4),
                        "pairs_per_s": round(B / med[m] * 1e3, 1), "rounds_ms": [round(x, 4) for x in res[m]]} for m in MODES}
        print("stage 1 %s (B = %d, 1 + %d titles, %d rounds x %d steps, median [min, max] ms per step):" % (key, B, Kn, a.rounds, a.steps))
        for m in MODES:
            print("  %-14s %7.3f ms  [%.3f, %.3f]  %7.1f pairs/s  %+6.1f %% vs joint_eval" % (
                m, med[m], min(res[m]), max(res[m]), B / med[m] * 1e3, 100 * (med[m] - med["joint_eval"]) / med["joint_eval"]))
        sys.stdout.flush()
        del s1
        torch.cuda.empty_cache()
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
