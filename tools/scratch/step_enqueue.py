"""Host time to ENQUEUE Engine.step alone (no forward, no backward) on the benchmark's engine: 4 layers, layers 2 and 3 trainable,
4 teachers, fp16, the loss scaler off as in host_overhead.py (its poll waits for the step two back, which would read as host
time).  Plain step(lr) and step with LAMB + clip + decay + average; 7 loops of 300 steps each, perf_counter in front of the final
synchronise, us per step.  TREE = another checkout's root to time its engine.py against this one's, a process per tree, the two
alternating (EXPERIMENTS.md item 77).      GPU box: python tools/scratch/step_enqueue.py [TREE]"""
import json, os, statistics, sys, time
ROOT = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tiny-newsrec_amd"))
import torch
import engine as E, hashinit
from schema import FULL, state_shapes
assert E.__file__.startswith(ROOT), E.__file__
cfg = E.EngineConfig(n_layers=4, trainable_layers=(2, 3), num_teachers=4)
eng = E.Engine(cfg, "cuda:0", max_batch=32, dtype="fp16")
eng.load_state_dict(hashinit.init_state_dict(1234, state_shapes(FULL, 4, cfg.D, 4)))
eng.scaler.enabled = False
eng.flat_g.copy_(torch.randn(eng.n_train, device="cuda:0") * 1e-3)
out = {"tree": ROOT}
for tag, kw in (("plain", {}), ("lamb_clip_decay_ema", dict(lamb=True, max_grad_norm=1.0, ema_decay=0.999, weight_decay=0.01))):
    for i in range(20):
        eng.step(lr=1e-4, **kw)
    torch.cuda.synchronize()
    reps = []
    for r in range(7):
        t0 = time.perf_counter()
        for i in range(300):
            eng.step(lr=1e-4, **kw)
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        reps.append((t1 - t0) / 300 * 1e6)
    out[tag + "_us"] = [round(x, 2) for x in reps]
    out[tag + "_median_us"] = round(statistics.median(reps), 2)
print(json.dumps(out))
