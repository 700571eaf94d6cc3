"""One data-parallel worker of tests/test_lamb_gpu.py, in the form of tests/workers/dp_rank.py (one process per rank, all on cuda:0,
torch.distributed over gloo): three LAMB steps through Engine.step(sync=..., lamb=True) on real backwards of each rank's half of
the batch, with clipping, the coupled decay and the average on, then a digest of every buffer the update writes and the trust
table.  Nothing about LAMB is communicated, so the digests of the ranks must agree."""
import hashlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tiny-newsrec_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def run(out_path, dtype, B, n_steps):
    import dist as D
    import engine as E
    import hashinit
    import synth
    from schema import FULL, state_shapes
    world, rank, _ = D.init("gloo")
    dev = "cuda:0"
    torch.cuda.set_device(0)
    nl, T_, n_news = 2, 2, 3000
    cfg = E.EngineConfig(n_layers=nl, trainable_layers=(0, 1), num_teachers=T_)
    b = B // world
    eng = E.Engine(cfg, dev, max_batch=b, dtype=dtype)
    eng.load_state_dict(hashinit.init_state_dict(7, state_shapes(FULL, nl, cfg.D, T_)))
    D.broadcast_flat([eng.flat[True], eng.flat[False]])
    eng.refresh_shadows(all_layers=True)
    gs = D.GradSync(eng.flat_g, eng.bucket_ranges(), world, force=True)
    d = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    comb, tabs = d(synth.news_table(7, n_news, cfg.L)), d(synth.teacher_tables(7, T_, n_news, cfg.D))
    hidx, mask, cidx, label = [d(x) for x in synth.impressions(8, B * n_steps, n_news, cfg.U, cfg.C)]
    p0 = eng.flat[True].clone()
    for st in range(n_steps):
        s = slice(st * B + rank * b, st * B + (rank + 1) * b)
        eng.forward_indexed(comb, hidx[s], mask[s], cidx[s], label[s], tabs)
        eng.backward(after_bucket=gs.launch if world > 1 else None)
        if world > 1:
            assert sorted(gs.pending) == list(range(len(gs.ranges)))
        eng.step(lr=1e-3, grad_scale=gs.scale, lr_bert=5e-4, sync=gs, lamb=True, weight_decay=0.01, max_grad_norm=0.05, ema_decay=0.9,
                 amsgrad=dtype == "fp16")
        assert not gs.pending
    torch.cuda.synchronize()
    if eng.scaler.enabled:
        eng.scaler.drain(eng)
    digest = lambda t: hashlib.sha256(t.detach().cpu().numpy().tobytes()).hexdigest()
    tr = eng.trust_ratios()
    out = {"p": digest(eng.flat[True]), "m": digest(eng.adam_m), "v": digest(eng.adam_v), "vmax": digest(eng.adam_vmax),
           "ema": digest(eng._ema), "w1": digest(eng.sh[1]["w1"]), "trust": {k: list(v) for k, v in tr.items()},
           "moved": not torch.equal(p0, eng.flat[True]), "skipped": eng.scaler.skipped, "steps": eng.step_count,
           "grad_norm": list(eng.grad_norm())}
    with open(out_path % rank, "w") as f:
        json.dump(out, f)
    D.barrier()
    if torch.distributed.is_initialized():
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    run(sys.argv[1], sys.argv[2], int(sys.argv[3]), int(sys.argv[4]))
