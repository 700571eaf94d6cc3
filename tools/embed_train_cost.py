"""What --train_embeddings costs: ms/step of the stage-2 step with EngineConfig(train_embeddings=) off and on, in ONE process on one
GPU, at bench.py's headline shape (4 layers, (2, 3) trainable, 4 teachers, B = 32) and at the 2-layer (0, 1) student; with the flag
on also the per-launch times of the entry points it adds (HIP events around each call, in extra steps after the timed region).
Same data as bench.py (synth tables, hash weights, resident table + indices, no de-duplication).  EXPERIMENTS.md records the output.

    python tools/embed_train_cost.py [--steps 30] [--warmup 5] [--batch 32] [--dtype fp16]      -> one JSON line"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tiny-newsrec_amd"))
sys.path.insert(0, ROOT)

import numpy as np   # noqa: E402
import torch         # noqa: E402

N_NEWS = 51282


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--dtype", choices=["bf16", "fp16"], default="fp16")
    a = ap.parse_args()
    import engine as E
    import hashinit
    import synth
    import tnr_hip as T
    from schema import FULL, state_shapes
    dev, seed, B, K, W = "cuda:0", 1234, a.batch, a.steps, a.warmup
    torch.cuda.set_device(0)
    base = E.EngineConfig()
    comb = torch.from_numpy(synth.news_table(seed, N_NEWS, base.L)).to(dev)
    tables = torch.from_numpy(synth.teacher_tables(seed, 4, N_NEWS, base.D)).to(dev)
    hidx, mask, cidx, label = [torch.from_numpy(np.ascontiguousarray(x)).to(dev)
                               for x in synth.impressions(seed + 1, (K + W) * B, N_NEWS, base.U, base.C)]
    out = {"dtype": a.dtype, "batch": B, "steps": K, "shapes": {}}
    for key, nl, tr in (("headline_4layer_23", 4, (2, 3)), ("student_2layer_01", 2, (0, 1))):
        sd = hashinit.init_state_dict(seed, state_shapes(FULL, nl, base.D, 4))
        res = {}
        for flag in (False, True):
            eng = E.Engine(E.EngineConfig(n_layers=nl, trainable_layers=tr, num_teachers=4, train_embeddings=flag), dev, max_batch=B,
                           dtype=a.dtype)
            eng.load_state_dict(sd)

            def step(i):
                s = slice((i % (K + W)) * B, (i % (K + W) + 1) * B)
                eng.forward_indexed(comb, hidx[s], mask[s], cidx[s], label[s], tables)
                eng.backward()
                eng.step(lr=1e-4)
            for i in range(W):
                step(i)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(W, W + K):
                step(i)
            torch.cuda.synchronize()
            r = {"ms_per_step": round(1e3 * (time.perf_counter() - t0) / K, 4), "n_train": int(eng.n_train),
                 "gradient_MB": round(4e-6 * eng.n_train, 1), "final_loss": round(float(eng.total_loss().item()), 5)}
            if flag:
                # three more steps with every call bracketed: the launches this flag adds are the embedding backward, the
                # scatter-sum, the fp32 column sums (the engine has no other fp32 tnr_colsum at this shape) and layer 0's qkv dgrad
                T.TIMED_ALL = []
                for i in range(3):
                    step(i)
                torch.cuda.synchronize()
                us = {}
                for e0, e1, name in T.TIMED_ALL:
                    us.setdefault(name, []).append(1e3 * e0.elapsed_time(e1))
                T.TIMED_ALL = None
                per_step = lambda n: round(sum(us.get(n, []) + us.get(n + "_f16", [])) / 3, 1)
                r["us_per_step"] = {"tnr_embed_ln_bwd_indexed": per_step("tnr_embed_ln_bwd_indexed"),
                                    "tnr_scatter_sum_rows": per_step("tnr_scatter_sum_rows"),
                                    "tnr_colsum (all)": per_step("tnr_colsum"), "tnr_amsgrad_step*": per_step("tnr_amsgrad_step_guarded") or per_step("tnr_amsgrad_step")}
                r["dx_workspace_MB"] = round(4e-6 * eng.dx_emb.numel(), 1)
            res["on" if flag else "off"] = r
            del eng
            torch.cuda.empty_cache()
        out["shapes"][key] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
