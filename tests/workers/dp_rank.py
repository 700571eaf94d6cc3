"""One data-parallel worker of tests/test_dp_gpu.py (started once per rank, all on cuda:0, torch.distributed over gloo so
that two ranks can share one GPU; device buckets are staged through host memory by dist.GradSync).

Each rank takes impressions [rank * B/W, (rank+1) * B/W) of a B-impression batch, runs Engine.forward / backward with the
bucketed all-reduce launched from the backward's after_bucket hook exactly as run.py / bench.py do, steps AMSGrad with the
1/W scale THROUGH Engine.step(sync=...) -- bucket by bucket, each optimiser slice behind its own in-flight collective
(GradSync keeps the gloo all-reduces asynchronous on pinned host mirrors) -- and dumps its summed gradient and its parameters.
mode "stage1": the same for post_train_kd.py's step (Stage1Engine: title pass writes the gradients, body pass accumulates and
fires the buckets).
mode "history": one long-lived Engine and one long-lived GradSync per rank through unlike steps of tests/history_ref.py, every
step against a fresh Engine + GradSync over the same process group (run_history).
mode "inbatch": two steps with in-batch negatives on, each rank on a half of its own (run_inbatch)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tiny-newsrec_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def run_stage1(out_path, dtype, B, n_steps):
    """post_train_kd.py's data-parallel step on a small Stage1Engine: 2 layers, 2 teachers, 1 + 3 titles of 24 tokens, bodies
    of 64; plain two-rate Adam as the notebook's cell 18."""
    import dist as D
    import hashinit
    import synth
    from schema import FULL, state_shapes
    from stage1 import Stage1Engine
    world, rank, _ = D.init("gloo")
    dev = "cuda:0"
    torch.cuda.set_device(0)
    nl, T_, n_docs, K, Lt, Lb = 2, 2, 500, 3, 24, 64
    b = B // world
    eng = Stage1Engine(n_layers=nl, trainable_layers=(0, 1), num_teachers=T_, npratio=K, title_len=Lt, body_len=Lb, device=dev,
                       batch=b, dtype=dtype)
    eng.load_state_dict({k: hashinit.init_tensor(11, k, tuple(shp)) for k, shp in eng.shapes.items()})
    t_eng = eng.title
    D.broadcast_flat([t_eng.flat[True], t_eng.flat[False]])
    t_eng.refresh_shadows(all_layers=True)
    eng.body.refresh_rel()
    gs = D.GradSync(t_eng.flat_g, eng.bucket_ranges(), world, force=True)
    d = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    titles, bodies = d(synth.news_table(11, n_docs, Lt)), d(synth.news_table(12, n_docs, Lb))
    tt, tb = d(synth.teacher_tables(11, T_, n_docs, 256)), d(synth.teacher_tables(12, T_, n_docs, 256))
    rs = np.random.RandomState(13)
    idx = d(rs.randint(1, n_docs, (B * n_steps, K + 1)).astype(np.int32))
    label = torch.zeros(b, dtype=torch.int64, device=dev)
    grads = []
    for st in range(n_steps):
        s = slice(st * B + rank * b, st * B + (rank + 1) * b)
        eng.forward_indexed(titles, bodies, idx[s], label, tt, tb)
        eng.backward(after_bucket=gs.launch if world > 1 else None)
        if st == 0:
            gs.wait()
            grads.append((t_eng.flat_g * gs.scale).cpu().numpy().copy())
            eng.step(1e-5, grad_scale=gs.scale, lr_bert=1e-6, amsgrad=False)
        else:
            eng.step(1e-5, grad_scale=gs.scale, lr_bert=1e-6, amsgrad=False, sync=gs)
            assert not gs.pending
            grads.append((t_eng.flat_g * gs.scale).cpu().numpy().copy())
    torch.cuda.synchronize()
    import engine as E
    np.savez(out_path % rank, grads=np.stack(grads), params=t_eng.flat[True].cpu().numpy(), gscale=np.float32(t_eng.gscale),
             head0=np.int64(t_eng.off(E.PFX + "dense.weight")))
    D.barrier()
    if torch.distributed.is_initialized():
        torch.distributed.destroy_process_group()


def run(out_path, dtype, B, n_steps, opts=None):
    """opts (optional, a JSON object): "engine" - further EngineConfig keywords (train_embeddings, vocab, max_pos; the weights
    are then hash-initialised over the engine's own shapes and the news table drawn from its vocabulary), "step" - further
    Engine.step keywords.  With it the dump also holds the parameters before the first step, the bucket indices the hook was
    called with, whether each backward's last call launched the last bucket behind the embedding scatter-sum, and grad_norm()
    of every step.  Without it nothing changes."""
    import dist as D
    import engine as E
    import hashinit
    import synth
    import tnr_hip as T
    from schema import FULL, state_shapes
    world, rank, _ = D.init("gloo")
    dev = "cuda:0"
    torch.cuda.set_device(0)
    nl, T_, n_news = 2, 2, 3000
    ekw, skw = (opts or {}).get("engine", {}), (opts or {}).get("step", {})
    cfg = E.EngineConfig(n_layers=nl, trainable_layers=(0, 1), num_teachers=T_, **ekw)
    b = B // world
    eng = E.Engine(cfg, dev, max_batch=b, dtype=dtype)
    if opts is None:
        eng.load_state_dict(hashinit.init_state_dict(7, state_shapes(FULL, nl, cfg.D, T_)))
    else:
        eng.load_state_dict(hashinit.init_state_dict(7, eng.shapes))
    D.broadcast_flat([eng.flat[True], eng.flat[False]])
    eng.refresh_shadows(all_layers=True)
    gs = D.GradSync(eng.flat_g, eng.bucket_ranges(), world, force=True)
    d = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    comb = d(synth.news_table(7, n_news, cfg.L) if opts is None else synth.news_table(7, n_news, cfg.L, vocab=cfg.vocab))
    tabs = d(synth.teacher_tables(7, T_, n_news, cfg.D))
    hidx, mask, cidx, label = [d(x) for x in synth.impressions(8, B * n_steps, n_news, cfg.U, cfg.C)]
    grads, more = [], {}
    hook = gs.launch
    if opts is not None:
        more.update(params0=eng.flat[True].cpu().numpy(), launched=[], embed_then_last_launch=[], clip=[],
                    n_buckets=np.int64(len(gs.ranges)), emb_end=np.int64(eng.bucket_ranges()[-1][1]))
        events, real = [], T.call

        def recorder(name, *a):
            events.append(name)
            return real(name, *a)

        def hook(bkt):
            events.append(bkt)
            more["launched"].append(bkt)
            gs.launch(bkt)
        T.call = recorder
    for st in range(n_steps):
        s = slice(st * B + rank * b, st * B + (rank + 1) * b)
        eng.forward_indexed(comb, hidx[s], mask[s], cidx[s], label[s], tabs)
        if opts is not None:
            del events[:]
        eng.backward(after_bucket=hook if world > 1 else None)
        if opts is not None and world > 1:
            more["embed_then_last_launch"].append("tnr_scatter_sum_rows" in events and events[-1] == len(gs.ranges) - 1)
        if world > 1:
            assert sorted(gs.pending) == list(range(len(gs.ranges)))      # every bucket's collective is in flight
        if st == 0:
            # what the buckets sum to, read BEFORE the optimiser (wait here, then step without sync); later steps take the
            # bucket-by-bucket path of run.py / bench.py
            gs.wait()
            grads.append((eng.flat_g * gs.scale).cpu().numpy().copy())
            eng.step(lr=1e-4, grad_scale=gs.scale, **skw)
        else:
            eng.step(lr=1e-4, grad_scale=gs.scale, sync=gs, **skw)
            assert not gs.pending
            grads.append((eng.flat_g * gs.scale).cpu().numpy().copy())
        if "max_grad_norm" in skw:
            more["clip"].append(eng.grad_norm())
    torch.cuda.synchronize()
    np.savez(out_path % rank, grads=np.stack(grads), params=eng.flat[True].cpu().numpy(), gscale=np.float32(eng.gscale),
             head0=np.int64(eng.off(E.PFX + "dense.weight")), **{k: np.asarray(v) for k, v in more.items()})
    D.barrier()
    if torch.distributed.is_initialized():
        torch.distributed.destroy_process_group()


def run_history(out_path, dtype):
    """Step-history independence at two real ranks: history_ref's model and feeds, rank r takes impressions [r b, (r + 1) b) of each
    feed (b = 3 of the full batch's 6, 2 of the short one's 4).  ONE Engine and ONE GradSync live through full_a -> short_a (the
    workspace re-laid, the pinned mirrors kept) -> full_b -> full_a at scaler.mult 0.5 -> full_a at 1.0; every backward launches its
    buckets through gs.launch, every optimiser step is step(sync=gs).  In front of each step the rank takes state_dict() and
    optimizer_state_dict(); behind it a FRESH Engine(max_batch=b) with a fresh GradSync is loaded from both and runs the same step
    over the same process group (both ranks in the same order, so the collectives pair up).  flat_g (the reduced gradient),
    flat[True], adam_m, adam_v and adam_vmax of the two must be torch.equal - a sum of two ranks is commutative, the collective
    adds no freedom - and no collective may be left pending.  Mismatches are collected and dumped (a rank that stopped at the first
    one would leave its peer waiting inside a collective); the parent asserts there are none."""
    sys.path.insert(0, ROOT)                # history_ref imports the oracle package
    import dist as D
    import engine as E
    import history_ref as HR
    world, rank, _ = D.init("gloo")
    assert world == 2
    dev = "cuda:0"
    torch.cuda.set_device(0)
    d = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    P = {k: d(v) for k, v in HR.weights().items()}
    comb, tabs = d(HR.news()), d(HR.teachers())
    per = {HR.B_FULL: HR.B_FULL // world, HR.B_SHORT: HR.B_SHORT // world}
    names = ("flat_g", "flat[True]", "adam_m", "adam_v", "adam_vmax")

    def make(b):
        e = E.Engine(E.EngineConfig(**HR.engine_kwargs()), dev, max_batch=b, dtype=dtype)
        return e, D.GradSync(e.flat_g, e.bucket_ranges(), world, force=True)

    def one(e, g, fid, mult, bad, who):
        b = per[HR.FEEDS[fid][0]]
        h, m, c, y = [d(x[rank * b:(rank + 1) * b]) for x in HR.feed(fid)]
        e.scaler.mult = mult
        e.forward_indexed(comb, h, m, c, y, tabs)
        e.backward(after_bucket=g.launch)
        if sorted(g.pending) != list(range(len(g.ranges))):
            bad.append("%s %s: collectives in flight behind backward: %s" % (who, fid, sorted(g.pending)))
        e.step(lr=HR.LR, grad_scale=g.scale, sync=g)
        if g.pending:
            bad.append("%s %s: collectives still pending behind step(sync=): %s" % (who, fid, sorted(g.pending)))
        torch.cuda.synchronize()
        return [x.clone() for x in (e.flat_g, e.flat[True], e.adam_m, e.adam_v, e.adam_vmax)]

    eng, gs = make(per[HR.B_FULL])
    eng.load_state_dict(P)
    D.broadcast_flat([eng.flat[True], eng.flat[False]])
    eng.refresh_shadows(all_layers=True)
    bad, moved = [], []
    for n, (fid, mult) in enumerate([("full_a", 1.0), ("short_a", 1.0), ("full_b", 1.0), ("full_a", 0.5), ("full_a", 1.0)]):
        sd, osd = eng.state_dict(), eng.optimizer_state_dict()
        p0 = eng.flat[True].clone()
        got = one(eng, gs, fid, mult, bad, "long-lived")
        fresh, fgs = make(per[HR.FEEDS[fid][0]])
        fresh.load_state_dict(sd)
        fresh.load_optimizer_state_dict(osd)
        want = one(fresh, fgs, fid, mult, bad, "fresh")
        for k, a, w in zip(names, got, want):
            if not torch.equal(a, w):
                bad.append("step %d (%s, mult %g): %s differs from the fresh engine's in %d elements, max |diff| %.3e" % (
                    n + 1, fid, mult, k, int((a != w).sum()), float((a.double() - w.double()).abs().max())))
        moved.append(not torch.equal(p0, got[1]) and bool(torch.isfinite(got[0]).all()) and float(got[0].abs().max()) > 0.0)
        del fresh, fgs, want
    eng.scaler.drain(eng)
    for msg in bad:
        print("HISTORY MISMATCH rank %d: %s" % (rank, msg))
    np.savez(out_path % rank, params=eng.flat[True].cpu().numpy(), skipped=np.int64(eng.scaler.skipped), steps=np.int64(eng.step_count),
             mismatches=np.int64(len(bad)), messages=np.asarray(bad, dtype=str), moved=np.asarray(moved), mult=np.float64(eng.scaler.mult))
    D.barrier()
    if torch.distributed.is_initialized():
        torch.distributed.destroy_process_group()


def run_inbatch(out_path, dtype):
    """In-batch negatives at two real ranks (tests/test_inbatch_steps_gpu.py): variants_ref's "att" model, rank 0 on
    inbatch_ref.engine_feed("e5"), rank 1 on "e5b" - unlike halves, five impressions each.  By design a rank ranks against its
    own batch only, so no collective is added and the reduced gradient is the sum of the two halves' own gradients.  Two steps
    with the option on, gs.launch the hook: behind the first backward the rank waits and dumps the reduced flat_g (times the
    scale) and its eligible counts, then steps; the second goes bucket by bucket through step(sync=gs)."""
    sys.path.insert(0, ROOT)                # variants_ref imports the oracle package
    import dist as D
    import engine as E
    import history_ref as HR
    import inbatch_ref as R
    import variants_ref as V
    world, rank, _ = D.init("gloo")
    assert world == 2
    dev = "cuda:0"
    torch.cuda.set_device(0)
    d = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    eng = E.Engine(E.EngineConfig(**V.engine_kwargs("att")), dev, max_batch=5, dtype=dtype)
    eng.load_state_dict({k: d(v) for k, v in V.weights("att").items()})
    D.broadcast_flat([eng.flat[True], eng.flat[False]])
    eng.refresh_shadows(all_layers=True)
    gs = D.GradSync(eng.flat_g, eng.bucket_ranges(), world, force=True)
    comb, tabs = d(HR.news()), d(HR.teachers())
    h, c, m, y = [d(x) for x in R.engine_feed(("e5", "e5b")[rank])]
    grads, counts, losses = [], [], []
    for st in range(2):
        ls, _ = eng.forward_indexed(comb, h, m, c, y, tabs, inbatch=True)
        losses.append(ls.cpu().numpy().copy())
        counts.append(eng.inbatch_counts().cpu().numpy().copy())
        eng.backward(after_bucket=gs.launch)
        assert sorted(gs.pending) == list(range(len(gs.ranges)))
        if st == 0:
            gs.wait()
            grads.append((eng.flat_g * gs.scale).cpu().numpy().copy())
            eng.step(lr=1e-4, grad_scale=gs.scale)
        else:
            eng.step(lr=1e-4, grad_scale=gs.scale, sync=gs)
            assert not gs.pending
            grads.append((eng.flat_g * gs.scale).cpu().numpy().copy())
    eng.scaler.drain(eng)
    torch.cuda.synchronize()
    np.savez(out_path % rank, grads=np.stack(grads), counts=np.stack(counts), losses=np.stack(losses), params=eng.flat[True].cpu().numpy(),
             scale=np.float64(gs.scale), skipped=np.int64(eng.scaler.skipped), steps=np.int64(eng.step_count))
    D.barrier()
    if torch.distributed.is_initialized():
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    if len(sys.argv) > 5 and sys.argv[5] == "inbatch":
        run_inbatch(sys.argv[1], sys.argv[2])
    elif len(sys.argv) > 5 and sys.argv[5] == "history":
        run_history(sys.argv[1], sys.argv[2])
    elif len(sys.argv) > 6:                   # stage 2 with options (the module docstring's argument list, then a JSON object)
        import json
        assert sys.argv[5] == "stage2"
        run(sys.argv[1], sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), json.loads(sys.argv[6]))
    else:
        (run_stage1 if len(sys.argv) > 5 and sys.argv[5] == "stage1" else run)(sys.argv[1], sys.argv[2], int(sys.argv[3]), int(sys.argv[4]))
