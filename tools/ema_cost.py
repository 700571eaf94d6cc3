"""What --ema_decay costs: the device time of Engine.step with the average off and on (alone, with the decay warm-up, and on top
of decay + schedule + clipping), fp16 and bf16, on one GPU at bench.py's headline shape (4 layers, (2, 3) trainable, 4 teachers,
B = 32) - and, with --parent_lib, against the step of the PARENT commit's library: the same engine code without the average,
run in a child process that loads that library instead of this tree's (the step's existing kernels are meant to be the ones they
were; this measures it).

flat_g is filled once with N(0, 1e-3^2) (no forward: the optimiser step does not care where its gradient came from); every
Engine.step is bracketed with a pair of events, as bench.py's step_breakdown_ms brackets its calls, so a figure is the time from
the step's first kernel to the end of the weight-copy refresh, launch gaps included.  The variants alternate in rounds within a
process, and each reports median and the 10th / 90th percentile over all its steps: compare differences against that spread.  The
derived expectation: the update moves 36 n bytes per launch with AMSGrad (5 reads, 4 writes of 4 bytes; run.py) and 28 n with plain
Adam (post_train_kd.py); the average adds one read and one write, 8 n: + 22.2 % / + 28.6 % of the UPDATE's bytes - the step's
other kernels (the fp16 scan, the weight-copy refresh) do not grow.  EXPERIMENTS.md records the output.

    python tools/ema_cost.py [--rounds 6] [--steps 40] [--batch 32] [--parent_lib PATH/libtnr_hip.so]      -> one JSON line
    python tools/ema_cost.py --kernel_sweep      -> the update kernel alone over buffer sizes inside and beyond the last-level cache"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tiny-newsrec_amd"))
sys.path.insert(0, ROOT)

import numpy as np   # noqa: E402
import torch         # noqa: E402

from adamw_cost import stats, timed   # noqa: E402


def measure(a, with_ema):
    import engine as E
    import hashinit
    from schema import FULL, state_shapes
    dev, seed = "cuda:0", 1234
    torch.cuda.set_device(0)
    cfg = E.EngineConfig()
    sd = hashinit.init_state_dict(seed, state_shapes(FULL, cfg.n_layers, cfg.D, cfg.T))
    out = {}
    for dtype in ("fp16", "bf16"):
        eng = E.Engine(cfg, dev, max_batch=a.batch, dtype=dtype)
        eng.load_state_dict(sd)
        eng.flat_g.copy_(torch.randn(eng.n_train, device=dev, generator=torch.Generator(device=dev).manual_seed(5)) * 1e-3)
        pos = 0
        for s_, e_ in sorted(eng.bucket_ranges()) + [(eng.n_train, eng.n_train)]:       # alignment gaps hold zeros after a backward
            eng.flat_g[pos:s_].zero_()
            pos = max(pos, e_)
        norm = 1e-3 * float(np.sqrt(eng.n_train))
        full = {"warmup_steps": 1000000, "lr_decay_steps": 2000000, "weight_decay": 0.01, "max_grad_norm": 0.5 * norm}
        variants = {"off": {}, "off_adam": {"amsgrad": False}, "decay_schedule_clip": dict(full)}
        if with_ema:
            variants.update({"ema": {"ema_decay": 0.999}, "ema_adam": {"ema_decay": 0.999, "amsgrad": False},
                             "ema_warmup": {"ema_decay": 0.999, "ema_warmup": True},
                             "ema_decay_schedule_clip": dict(full, ema_decay=0.999)})
        us = {k: [] for k in variants}
        for k, kw in variants.items():                                              # warm-up: every variant's kernels and buffers
            timed(lambda: eng.step(1e-4, **kw), 5)
        for _ in range(a.rounds):
            for k, kw in variants.items():
                us[k] += timed(lambda: eng.step(1e-4, **kw), a.steps)
        r = {k: stats(v) for k, v in us.items()}
        r["n_train"], r["gradient_MB"] = int(eng.n_train), round(4e-6 * eng.n_train, 1)
        out[dtype] = r
        del eng
        torch.cuda.empty_cache()
    return out


def kernel_sweep(a):
    """The update kernel alone, without and with the average, at buffer sizes from well inside the 256 MB last-level cache to far
    beyond it (the step's other kernels and its launch structure are out of the picture): ONE launch over n elements, AMSGrad and
    plain Adam, the two entry points alternating; median microseconds, the bytes moved per second, and the ratio beside the derived
    (36 + 8) / 36 and (28 + 8) / 28."""
    import tnr_hip as T
    dev = "cuda:0"
    torch.cuda.set_device(0)
    out = {}
    for n in (2 << 20, 8 << 20, 14884864, 48 << 20):
        g = torch.Generator(device=dev).manual_seed(5)
        p, e = torch.randn(n, device=dev, generator=g), torch.randn(n, device=dev, generator=g)
        gr = torch.randn(n, device=dev, generator=g) * 1e-3
        m, v, x = torch.zeros(n, device=dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev)
        r = {}
        for ams in (True, False):
            head = (p, gr, m, v, x if ams else None, n, 3, 1e-4, 1e-4, 1e-4, 0.9, 0.999, 1e-8, 1.0, 0.0, None, 0, None, 0, 0, None)
            plain = lambda: T.call("tnr_adamw_step", *head)
            ema = lambda: T.call("tnr_adamw_step_ema", *head, e, 1e-3, 1e-3, 1e-3)
            us = {"plain": [], "ema": []}
            timed(plain, 5), timed(ema, 5)
            for _ in range(a.rounds):
                us["plain"] += timed(plain, a.steps)
                us["ema"] += timed(ema, a.steps)
            s = {k: stats(w) for k, w in us.items()}
            b = 36 if ams else 28
            r["amsgrad" if ams else "adam"] = {
                "plain": s["plain"], "ema": s["ema"], "ratio": round(s["ema"]["median_us"] / s["plain"]["median_us"], 4),
                "derived_ratio": round((b + 8) / b, 4), "plain_TB_s": round(b * n / s["plain"]["median_us"] * 1e-6, 2),
                "ema_TB_s": round((b + 8) * n / s["ema"]["median_us"] * 1e-6, 2),
                "footprint_MB": [round(4e-6 * n * (b // 8 + 1)), round(4e-6 * n * (b // 8 + 2))]}
        out[str(n)] = r
        del p, e, gr, m, v, x
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel_sweep", action="store_true", help="time the update kernel alone, without and with the average, over a range "
                    "of buffer sizes, instead of Engine.step")
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--steps", type=int, default=40, help="steps per variant and round")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--parent_lib", default=None, help="libtnr_hip.so built from the parent commit: its step is measured in a child process")
    ap.add_argument("--as_parent", default=None, help=argparse.SUPPRESS)       # the child: load this library, measure the variants without the average
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/ema_cost.py measures on the GPU: none found")
    if a.as_parent:
        import tnr_hip as T
        T.LIB_PATH = os.path.abspath(a.as_parent)
        T._SIG.pop("tnr_adamw_step_ema")                # the parent's library does not export it
        print(json.dumps(measure(a, with_ema=False)))
        return
    if a.kernel_sweep:
        print(json.dumps({"rounds": a.rounds, "steps_per_round": a.steps, "kernel": kernel_sweep(a)}))
        return
    out = {"batch": a.batch, "rounds": a.rounds, "steps_per_round": a.steps, "step": measure(a, with_ema=True)}
    if a.parent_lib:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--rounds", str(a.rounds), "--steps", str(a.steps), "--batch",
                            str(a.batch), "--as_parent", a.parent_lib], capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            raise SystemExit("the parent's measurement failed:\n" + (r.stdout + r.stderr)[-2000:])
        out["parent_step"] = json.loads(r.stdout.strip().splitlines()[-1])
    for dtype, r in out["step"].items():
        bases = {"this build's": r}
        if a.parent_lib:
            bases["parent's"] = out["parent_step"][dtype]
        cmp_ = {}
        for k, base, derived in (("ema", "off", 8.0 / 36.0), ("ema_warmup", "off", 8.0 / 36.0), ("ema_adam", "off_adam", 8.0 / 28.0),
                                 ("ema_decay_schedule_clip", "decay_schedule_clip", 8.0 / 36.125)):
            for whose, b in bases.items():
                cmp_["%s over %s %s" % (k, whose, base)] = {
                    "ratio": round(r[k]["median_us"] / b[base]["median_us"], 4),
                    "extra_us": round(r[k]["median_us"] - b[base]["median_us"], 1),
                    "base_p10_p90_spread_us": round(b[base]["p90_us"] - b[base]["p10_us"], 1),
                    "derived_extra_update_bytes": round(derived, 4)}
        if a.parent_lib:
            for k in ("off", "off_adam", "decay_schedule_clip"):
                b = out["parent_step"][dtype][k]
                cmp_["%s over parent's %s" % (k, k)] = {"ratio": round(r[k]["median_us"] / b["median_us"], 4),
                                                        "inside_parent_p10_p90": bool(b["p10_us"] <= r[k]["median_us"] <= b["p90_us"])}
        r["compare"] = cmp_
    print(json.dumps(out))


if __name__ == "__main__":
    main()
