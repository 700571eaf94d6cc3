"""Entry point with the reference's interface (Tiny-NewsRec/run.py:463-472): python run.py --mode train ...
Training loop = run.py:20-216 (step order fwd -> acc -> zero_grad -> backward -> step, log line format,
epoch-end checkpoint dict and file name, max_steps_per_epoch break), on the HIP engine with RCCL replacing
horovod.  --mode test / get_teacher_emb are the forward-only paths of SURVEY.md section 8-f N2."""
import logging
import os
import sys
import pickle
import time

import numpy as np
import torch

import utils
from parameters import parse_args


def _load_inputs(args):
    """news table + teacher embeddings (run.py:46-53, 73-74) or their synthetic stand-ins."""
    if args.synthetic:
        import synth
        n = 51282
        comb = synth.news_table(1234, n, args.num_words_title)
        tables = list(synth.teacher_tables(1234, args.num_teachers, n, args.news_dim)) if args.num_teachers else []
        return {"N%d" % i: i for i in range(1, n + 1)}, comb, tables, {}, {}
    from preprocess import get_doc_input_bert, read_news_bert
    news, news_index, cat, sub = read_news_bert(os.path.join(args.train_data_dir, "news.tsv"), args, mode="train")
    title, mask, _, _ = get_doc_input_bert(news, news_index, cat, sub, args)
    tables = []
    for p in args.teacher_emb_paths[:args.num_teachers]:
        with open(p, "rb") as f:
            tables.append(np.asarray(pickle.load(f), dtype=np.float32))
    return news_index, np.concatenate([title, mask], axis=-1), tables, cat, sub


def _train_flags(args, world):
    """The flags a --save_optimizer checkpoint records (train_state["flags"]): what a --resume run compares its own against.
    `optimizer` is recorded when it is not the default: a checkpoint of an adam run holds the flags it always held, and a
    checkpoint without the key was written by adam."""
    names = ("lr", "pretrain_lr", "weight_decay", "warmup_steps", "lr_decay_steps", "ema_decay", "ema_warmup", "grad_accum_steps",
             "max_grad_norm", "batch_size", "dtype")
    flags = {k: getattr(args, k) for k in names}
    flags["world"] = world
    if getattr(args, "inbatch_negatives", False):        # recorded when on, as `optimizer` is: an older checkpoint ran without it
        flags["inbatch_negatives"] = True
    if getattr(args, "optimizer", "adam") != "adam":
        flags["optimizer"] = args.optimizer
    return flags


def train(args):
    if getattr(args, "resume", False) and not args.load_ckpt_name:          # (parse_args refuses it too; args may come from elsewhere)
        raise ValueError("--resume True needs --load_ckpt_name (the checkpoint a --save_optimizer True run wrote)")
    import dist
    from dataloader import DataLoaderTrain, IndexBatch
    from model_bert import Model, ModelBert, TnrAdam
    from streaming import get_stat, get_worker_files
    size, rank, local = utils.init_hvd_cuda(args.enable_hvd, args.enable_gpu)
    assert args.enable_gpu, "the HIP path needs a GPU (there is no CPU fallback)"
    # the loader's producer thread (TSV decode) and this thread (kernel launches) share the GIL: with the default 5 ms switch
    # interval the launching thread can sit out a whole 3 ms step behind the decoder and the GPU queue runs dry
    sys.setswitchinterval(2e-4)
    news_index, news_combined, teacher_embs, category_dict, subcategory_dict = _load_inputs(args)
    # --num_teachers 0 is PLM-NR/run.py's train(): the same encoders with plain CE (ModelBert), checkpoints with PLM-NR's
    # key names, and -- with --use_pretrain_model -- its two learning rates (PLM-NR/run.py:56-106).  Tiny-NewsRec's own
    # Model cannot be built without teachers, so the flag value is free for this.
    plmnr = args.num_teachers == 0
    if size > 1:
        # beside the CUs an overlapped gradient all-reduce holds, a late workgroup of the weight-gradient kernel costs one work
        # unit: two units per workgroup halve that (engine.Engine.WGRAD_UNITS; set before the engine sizes its slab workspace)
        import engine as E
        E.Engine.WGRAD_UNITS = 2
    model = ModelBert(args) if plmnr else Model(args)
    eng = model.engine
    for index in eng.cfg.trainable_layers:                                   # run.py:108
        logging.info(f"finetune block {index}")
    if eng.cfg.train_embeddings:
        logging.info("finetune embeddings")
    sd = model.state_dict()
    pretrained = False
    if args.synthetic:
        import hashinit
        pfx = "student." if plmnr else ""
        sd = {k: torch.from_numpy(hashinit.init_tensor(1234, pfx + k, tuple(v.shape))) for k, v in sd.items()}
    elif plmnr:
        if args.use_pretrain_model:                                          # PLM-NR/run.py:56-70 (first-stage student -> this model)
            for k, v in torch.load(args.pretrain_model_path, map_location="cpu")["model_state_dict"].items():
                k2 = k[len("student."):] if k.startswith("student.") else None
                if k2 in sd:
                    sd[k2] = v
                    pretrained = True
    else:
        for i, ck in enumerate(args.teacher_ckpts[:args.num_teachers]):      # run.py:61-70
            for k, v in torch.load(ck, map_location="cpu")["model_state_dict"].items():
                if k.startswith("user_encoder"):
                    sd[".".join(["teachers", str(i)] + k.split(".")[1:])] = v
        if args.use_pretrain_model:                                          # run.py:76-85
            for k, v in torch.load(args.pretrain_model_path, map_location="cpu")["model_state_dict"].items():
                if k.startswith("student"):
                    sd[k] = v
    model.load_state_dict(sd)
    loaded = None
    if args.load_ckpt_name is not None:                                      # run.py:125-129
        ck = utils.get_checkpoint(args.model_dir, args.load_ckpt_name)
        loaded = torch.load(ck, map_location="cpu")
        model.load_state_dict(loaded["model_state_dict"])
        logging.info(f"Model loaded from {ck}")
        if args.ema_decay > 0 and "ema_state_dict" in loaded:      # the average resumes; without one it starts from the loaded parameters
            model.load_ema_state_dict(loaded["ema_state_dict"])
            eng.ema_updates = int(loaded.get("ema", {}).get("updates", 0))
            logging.info(f"EMA of the weights resumed from {ck} ({eng.ema_updates} updates)")
    dist.broadcast_flat([eng.flat[True], eng.flat[False]])                   # hvd.broadcast_parameters, run.py:142
    eng.refresh_shadows(all_layers=True)
    sync = dist.GradSync(eng.flat_g, eng.bucket_ranges(), size)             # hvd.DistributedOptimizer(Average), :145-149
    model._after_bucket = sync.launch if size > 1 else None
    optimizer = TnrAdam(model, args.lr, sync if size > 1 else None,
                        pretrain_lr=args.pretrain_lr if (plmnr and pretrained) else None,      # PLM-NR/run.py:94-106
                        pretrained_heads=plmnr and pretrained, max_grad_norm=args.max_grad_norm,
                        weight_decay=args.weight_decay, warmup_steps=args.warmup_steps, lr_decay_steps=args.lr_decay_steps,
                        ema_decay=args.ema_decay, ema_warmup=args.ema_warmup, grad_accum_steps=args.grad_accum_steps,
                        optimizer=args.optimizer)
    accum_logged = False
    first_epoch = args.start_epoch
    if args.resume:
        # the run that wrote the checkpoint goes on: optimiser state behind the parameters and the average (above), then the epoch
        if "optimizer_state_dict" not in loaded:
            raise KeyError(f"--resume True: {ck} holds no optimizer_state_dict (it was not written with --save_optimizer True)")
        optimizer.load_state_dict(loaded["optimizer_state_dict"])
        # every rank read the same file; one source for the buffers all the same (hvd.broadcast_optimizer_state, run.py:143)
        dist.broadcast_flat([eng.adam_m, eng.adam_v, eng.adam_vmax] + ([eng._ema] if eng._ema is not None else []))
        ts = loaded["train_state"]
        first_epoch = int(ts["epoch"])
        if args.start_epoch not in (0, first_epoch):
            raise ValueError(f"--resume True: {ck} was written at the end of epoch {first_epoch}, --start_epoch says {args.start_epoch}")
        mine = dict(_train_flags(args, size), optimizer=args.optimizer, inbatch_negatives=bool(getattr(args, "inbatch_negatives", False)))
        for k, v in dict(ts.get("flags", {}), optimizer=ts.get("flags", {}).get("optimizer", "adam"),
                         inbatch_negatives=ts.get("flags", {}).get("inbatch_negatives", False)).items():
            if k in mine and mine[k] != v:
                logging.warning(f"--resume True: --{k} is {mine[k]}, the run that wrote {ck} had {v}" if k != "world" else
                                f"--resume True: {size} worker(s), the run that wrote {ck} had {v}")
        logging.info(f"[{rank}] Resumed from {ck}: {eng.step_count} updates taken, continuing at epoch {first_epoch}")
        if args.epochs <= first_epoch:
            logging.info(f"[{rank}] --epochs {args.epochs} is not beyond the saved epoch {first_epoch}: nothing left to train")
            return

    if args.synthetic:
        import synth
        steps = min(args.max_steps_per_epoch, 200)
        steps_cap = steps
        hidx, mask, cidx, label = [torch.from_numpy(x).cuda() for x in
                                   synth.impressions(77 + rank, steps * args.batch_size, len(news_index), args.user_log_length, args.npratio + 1)]
        B = args.batch_size
        dev_news = torch.from_numpy(news_combined).cuda()
        dev_tab = torch.from_numpy(np.stack(teacher_embs, 0)).cuda() if teacher_embs else None
        plans = [None] * steps
        if args.dedup_news:
            from dedup import build_plan
            hn, cn = hidx.cpu().numpy(), cidx.cpu().numpy()
            plans = [build_plan(hn[i * B:(i + 1) * B], cn[i * B:(i + 1) * B]) for i in range(steps)]
            plans = [p.to("cuda") if p is not None else None for p in plans]
        batches = lambda: (IndexBatch((hidx[i * B:(i + 1) * B], mask[i * B:(i + 1) * B], cidx[i * B:(i + 1) * B],
                                       label[i * B:(i + 1) * B], plans[i])) for i in range(steps))
    else:
        stat = get_stat(args.train_data_dir, args.filename_pat)
        paths = get_worker_files(args.train_data_dir, rank, size, args.filename_pat, args.enable_shuffle, 0)
        n = sum(stat[f] for f in paths)
        logging.info("[{}] contains {} samples {} steps".format(rank, n, n // args.batch_size))
        steps_cap = None          # per epoch, below: the loader re-shards the files every epoch
        loader = DataLoaderTrain(teacher_embs=teacher_embs, news_index=news_index, news_combined=news_combined, word_dict=None,
                                 data_dir=args.train_data_dir, filename_pat=args.filename_pat, args=args, world_size=size,
                                 worker_rank=rank, cuda_device_idx=local, enable_prefetch=True, enable_shuffle=True,
                                 enable_gpu=True, resident=args.resident_tables)
        dev_news, dev_tab = getattr(loader, "dev_news", None), loader.dev_tables
        # the loader itself, not iter(loader): the epoch loop's enumerate() calls __iter__, and every call of it starts an epoch
        # (a producer, a re-sharding, the counter + 1) - two calls per epoch made the counter run two ahead of the seed epoch_cap()
        # asks about, so the cap belonged to another file set than the one the epoch read
        batches = lambda: loader
        if args.resume:
            loader.epoch = first_epoch - 1       # shard assignment and shuffle seeds go on as in the uninterrupted run

        def epoch_cap():
            # uneven shards: every rank runs the step count the shortest shard of THIS epoch allows (the loader re-shards the
            # files with the epoch number as shuffle seed; the last batch may be short, streaming.py:76), otherwise the rank
            # that finishes first leaves the others waiting in the gradient all-reduce
            cap = dist.min_over_ranks(loader.next_epoch_batches(stat))
            if size > 1:
                logging.info("[{}] {} steps this epoch on every rank (shortest shard)".format(rank, cap))
            return cap

    if args.cache_frozen_layers and dev_news is not None and eng.build_frozen_cache(dev_news):
        logging.info("[%d] frozen layers 0..%d cached for %d news (%.2f GB)" % (
            rank, eng.lo - 1, dev_news.shape[0], eng.fcache[0].numel() * 4 / 1e9))
    valid = _Validation(args, size, rank, local) if getattr(args, "valid_data_dir", None) else None
    valid_steps = getattr(args, "valid_steps", 0) if valid is not None else 0

    def model_ckpt():
        """The epoch checkpoint's model keys (run.py:205-214, plus the average of an --ema_decay run)."""
        ck = {"model_state_dict": {k: v.cpu() for k, v in model.state_dict().items()},
              "category_dict": category_dict, "word_dict": None, "subcategory_dict": subcategory_dict}
        esd = model.ema_state_dict() if args.ema_decay > 0 else None
        if esd is not None:          # --ema_decay: the averaged model beside the trained one, which stays what the reference loads
            ck["ema_state_dict"] = {k: v.cpu() for k, v in esd.items()}
            ck["ema"] = {"decay": args.ema_decay, "warmup": bool(args.ema_warmup), "updates": eng.ema_updates}
        return ck

    def validate(epoch, batch):
        """Every rank: the held-out metrics of the weights as they are now; rank 0 keeps the best of the run in best.pt."""
        v = valid.run(eng, epoch, batch)
        if rank == 0 and valid.improved(v):
            os.makedirs(args.model_dir, exist_ok=True)
            best_path = os.path.join(args.model_dir, "best.pt")
            torch.save(dict(model_ckpt(), valid=v), best_path)
            logging.info(f"Best validation AUC so far: model saved to {best_path}")
        return v

    inbatch = bool(getattr(args, "inbatch_negatives", False))
    logging.info("Training...")
    for ep in range(first_epoch, args.epochs):
        loss_sum, acc_sum, t0 = torch.zeros((), device="cuda"), torch.zeros((), device="cuda"), time.time()
        if not args.synthetic:
            steps_cap = epoch_cap()
        optimizer.reset_window()         # --grad_accum_steps: a window never spans two epochs
        n_batches, last_valid = 0, None
        left_over = min(args.max_steps_per_epoch + 1, steps_cap) % args.grad_accum_steps
        if left_over and not accum_logged:
            accum_logged = True
            logging.info("[{}] --grad_accum_steps {}: the last {} batch(es) of an epoch of {} fall outside a full window and "
                         "update nothing".format(rank, args.grad_accum_steps, left_over, min(args.max_steps_per_epoch + 1, steps_cap)))
        for cnt, batch in enumerate(batches()):
            if cnt > args.max_steps_per_epoch or cnt >= steps_cap:
                break
            if isinstance(batch, IndexBatch):
                h, m, c, y, plan = batch
                if plmnr:
                    total, y_student = model.forward_indexed(dev_news, h, m, c, y, plan, inbatch=inbatch)
                else:
                    total, distill, emb, target, y_student = model.forward_indexed(dev_news, h, m, c, y, dev_tab, plan, inbatch=inbatch)
            elif plmnr:
                h, m, c, y = batch[:4]
                total, y_student = model(h, m, c, y, plan=getattr(batch, "plan", None), inbatch_ids=batch.ids if inbatch else None)
            else:
                h, m, c, y, th, tc = batch
                total, distill, emb, target, y_student = model(h, m, c, y, th, tc, plan=getattr(batch, "plan", None),
                                                               inbatch_ids=batch.ids if inbatch else None)
            loss_sum += total.detach()
            acc_sum += utils.acc(y, y_student)
            optimizer.zero_grad()
            total.backward()
            optimizer.step()
            if cnt % args.log_steps == 0:
                d = max(cnt, 1)
                sc = eng.scaler          # fp16: steps whose 16-bit backward overflowed are skipped on the device (engine.LossScaler)
                gn = eng.grad_norm() if args.max_grad_norm > 0 else None     # this step's norm after the all-reduce, and its clip
                tr = eng.trust_ratios() if args.optimizer == "lamb" else None      # this step's LAMB ratios over the adapted tensors
                if tr:
                    tv = sorted(t for t, _, _ in tr.values())
                    logging.info("[{}] trust ratio min {:g} / median {:g} / max {:g} over {} tensors".format(
                        rank, tv[0], tv[len(tv) // 2], tv[-1], len(tv)))
                if inbatch:      # this step's count, read back on log steps only
                    logging.info("[{}] in-batch negatives: {:.1f} eligible per impression (target loss over 1 + {} + those)".format(
                        rank, eng.inbatch_counts().float().mean().item(), args.npratio))
                logging.info("[{}] Ed: {}, train_loss: {:.5f}, acc: {:.5f}, {:.1f} impressions/s{}{}{}".format(
                    rank, cnt * args.batch_size, loss_sum.item() / d, acc_sum.item() / d,
                    size * cnt * args.batch_size / max(time.time() - t0, 1e-9),
                    ", loss scale {:g}, {} steps skipped (fp16 overflow)".format(eng.gscale, sc.skipped) if sc.enabled and sc.skipped else "",
                    ", grad norm {:g} (clip x{:.3g})".format(*gn) if gn is not None else "",
                    # the host's schedule multiplier of the last step (the device may be up to two skipped steps behind it)
                    ", lr x{:.4g}".format(eng.lr_scale) if eng.lr_scale is not None else ""))
            n_batches = cnt + 1
            if valid_steps and n_batches % valid_steps == 0:     # a multiple of --grad_accum_steps: behind an update, never inside a window
                last_valid = validate(ep + 1, n_batches)
        print(ep + 1)
        if eng.scaler.enabled:
            eng.scaler.drain(eng)        # the epoch's last two overflow answers, before the step count goes into a log line or a file
        if valid is not None:            # every rank, before the checkpoint; the epoch's last batch may just have been validated
            if last_valid is None or last_valid["batch"] != n_batches:
                last_valid = validate(ep + 1, n_batches)
        if rank == 0:                                                        # run.py:205-214
            os.makedirs(args.model_dir, exist_ok=True)
            ckpt_path = os.path.join(args.model_dir, f"epoch-{ep + 1}.pt")
            ckpt = model_ckpt()
            if valid is not None:
                ckpt["valid"] = dict(last_valid, updates=eng.step_count)
            if args.save_optimizer:      # what --resume True continues from (after the drain above: the counts are final)
                optimizer.reset_window()     # a partial window at the end of the epoch is dropped, as the next epoch's start drops it
                ckpt["optimizer_state_dict"] = optimizer.state_dict()
                ckpt["train_state"] = {"epoch": ep + 1, "updates": eng.step_count, "flags": _train_flags(args, size)}
            torch.save(ckpt, ckpt_path)
            logging.info(f"Model saved to {ckpt_path}")
    if not args.synthetic:
        loader.join()


def _news_table(args, data_dir, mode):
    from preprocess import get_doc_input_bert, read_news_bert
    if mode == "train":
        news, news_index, cat, sub = read_news_bert(os.path.join(data_dir, "news.tsv"), args, mode="train")
    else:
        news, news_index = read_news_bert(os.path.join(data_dir, "news.tsv"), args, mode="test")
        cat, sub = {}, {}
    title, mask, _, _ = get_doc_input_bert(news, news_index, cat, sub, args)
    return news_index, np.concatenate([title, mask], axis=-1).astype(np.int32)


def _forward_engine(args, n_layers, sd, add_prefix=""):
    """Frozen engine (no teachers, nothing trainable).  sd: reference Model keys ("student. ...") or, with
    add_prefix="student.", PLM-NR ModelBert keys ("news_encoder. ...", "user_encoder. ...")."""
    import types
    import engine as E
    from model_bert import engine_config_from_args
    a = types.SimpleNamespace(**vars(args))
    a.num_student_layers, a.bert_trainable_layer = n_layers, []
    a.train_embeddings = False
    cfg = engine_config_from_args(a, num_teachers=0)
    eng = E.Engine(cfg, "cuda:%d" % torch.cuda.current_device(), max_batch=args.batch_size, dtype=getattr(args, "dtype", "fp16"))
    src = {add_prefix + k: v for k, v in sd.items()}
    eng.load_state_dict({k: src[k] for k in eng.shapes})
    return eng


class _Validation:
    """--valid_data_dir: the held-out set of a training run.  Its news table is read and uploaded once; run() encodes it with the
    live student through the training engine's own encode_news (the frozen-layer cache is keyed by the training table's address,
    so this table never hits it, and a forward-only pass leaves nothing behind that a training step reads), takes the user
    vectors from its user_vectors and the metrics from the device path of test mode, sharded over the ranks by DataLoaderTest
    and reduced as test() reduces them."""

    def __init__(self, args, size, rank, local):
        self.args, self.size, self.rank, self.local = args, size, rank, local
        self.news_index, comb = _news_table(args, args.valid_data_dir, "test")
        self.dev_news = torch.from_numpy(comb).cuda()
        self.best = None
        logging.info("[{}] validation on {}: {} news".format(rank, args.valid_data_dir, comb.shape[0]))

    def run(self, eng, epoch, batch):
        """-> the `valid` record of the checkpoints; the same on every rank."""
        from dataloader import DataLoaderTest
        args = self.args
        news_scoring = eng.encode_news(self.dev_news)
        loader = DataLoaderTest(news_index=self.news_index, data_dir=args.valid_data_dir,
                                filename_pat=getattr(args, "valid_filename_pat", "behaviors_*.tsv"), args=args, world_size=self.size,
                                worker_rank=self.rank, cuda_device_idx=self.local, enable_prefetch=True, enable_shuffle=False,
                                enable_gpu=True)
        sums, n_local, scored = _impression_loop(eng, news_scoring, loader, self.rank, args.log_steps, device_metrics=True)
        t = _reduce_metrics(sums, n_local, self.size, extra=(scored,))
        if t[0] == 0:
            raise ValueError(f"--valid_data_dir {args.valid_data_dir}: no impressions match {getattr(args, 'valid_filename_pat', None)}")
        m = t[1:5] / t[0]                # by the SAMPLE count, as test mode's final line (run.py:377-379)
        v = {"auc": float(m[0]), "mrr": float(m[1]), "ndcg5": float(m[2]), "ndcg10": float(m[3]), "seen": int(t[0]),
             "scored": int(t[5]), "epoch": epoch, "batch": batch, "updates": eng.step_count}
        logging.info("[{}] Valid: epoch {} batch {}: {} ({} impressions, {} scored)".format(
            self.rank, epoch, batch, "\t".join("{:0.2f}".format(x * 100) for x in m), v["seen"], v["scored"]))
        return v

    def improved(self, v):
        if self.best is not None and not v["auc"] > self.best:
            return False
        self.best = v["auc"]
        return True


def get_teacher_emb(args):
    """run.py:382-460: every train news through each teacher's news encoder -> pickled (n+1, D) float32 tables."""
    utils.init_hvd_cuda(False, args.enable_gpu)
    _, news_combined = _news_table(args, args.train_data_dir, "train")
    dev_news = torch.from_numpy(news_combined).cuda()
    for ckpt_path, out_path in zip(args.teacher_ckpts, args.teacher_emb_paths):
        sd = torch.load(ckpt_path, map_location="cpu")["model_state_dict"]          # PLM-NR keys: news_encoder.* / user_encoder.*
        eng = _forward_engine(args, args.num_hidden_layers, sd, add_prefix="student.")
        logging.info(f"loaded teacher model: {ckpt_path}")
        news_scoring = eng.encode_news(dev_news).cpu().numpy()
        logging.info("news scoring num: {}".format(news_scoring.shape[0]))
        with open(out_path, "wb") as f:
            pickle.dump(news_scoring, f)
        logging.info(f"teacher embedding saved at {out_path}")
        del eng
        torch.cuda.empty_cache()


def test(args, collect=None):
    """run.py:219-379: encode all test news once, user vectors per impression batch, host metrics, scalar all-reduce.
    collect: optional list that receives, per impression in file order, (scores, labels) - the reference keeps only the sums;
    the quality tests compare the per-impression rankings with the reference's."""
    import dist
    from dataloader import DataLoaderTest
    size, rank, local = utils.init_hvd_cuda(args.enable_hvd, args.enable_gpu)
    ckpt_path = utils.get_checkpoint(args.model_dir, args.load_ckpt_name) if args.load_ckpt_name else utils.latest_checkpoint(args.model_dir)
    assert ckpt_path is not None, "No ckpt found"
    ckpt = torch.load(ckpt_path, map_location="cpu")
    if getattr(args, "use_ema", False):
        if "ema_state_dict" not in ckpt:
            raise KeyError(f"--use_ema True: {ckpt_path} holds no ema_state_dict (it was not trained with --ema_decay)")
        sd = ckpt["ema_state_dict"]
    else:
        sd = ckpt["model_state_dict"]
    eng = _forward_engine(args, args.num_student_layers, sd)
    logging.info(f"Model loaded from {ckpt_path}" + (" (the EMA of the weights)" if getattr(args, "use_ema", False) else ""))
    news_index, news_combined = _news_table(args, args.test_data_dir, "test")
    news_scoring = eng.encode_news(torch.from_numpy(news_combined).cuda())
    logging.info("news scoring num: {}".format(news_scoring.shape[0]))
    loader = DataLoaderTest(news_index=news_index, data_dir=args.test_data_dir, filename_pat=args.filename_pat, args=args,
                            world_size=size, worker_rank=rank, cuda_device_idx=local, enable_prefetch=True,
                            enable_shuffle=False, enable_gpu=True)
    sums, n_local, cnt_metric = _impression_loop(eng, news_scoring, loader, rank, args.log_steps,
                                                 getattr(args, "device_metrics", False), collect)
    logging.info("[{}] local_sample_num: {}".format(rank, n_local))
    t = _reduce_metrics(sums, n_local, size)
    if rank == 0:
        # the reference divides the metric sums by the SAMPLE count (run.py:377-379), impressions skipped above included
        logging.info("[{}] Ed: {}: {}".format(rank, int(t[0]), "\t".join("{:0.2f}".format(x * 100) for x in t[1:5] / t[0])))
    return sums, n_local, cnt_metric


def _impression_loop(eng, news_scoring, loader, rank, log_steps, device_metrics=False, collect=None):
    """The impression loop of test mode (run.py:332-366) over one pass of an eval loader, which it joins
    -> (sums of AUC / MRR / nDCG@5 / nDCG@10 over the impressions scored, impressions seen, impressions scored), this rank's.
    Host form (the reference's): user vectors to the host, per impression one numpy dot product per candidate and metrics.py.
    device_metrics: one Engine.evaluate per batch adds to six doubles on the device, read back for a log line and at the end -
    no host copy of news_scoring, no per-impression host work.  collect receives (scores, labels) per impression in file order:
    the host's dot products, or the device's own scores."""
    sums, n_local, cnt_metric = np.zeros(4), 0, 0
    if device_metrics:
        acc = torch.zeros(6, dtype=torch.float64, device=news_scoring.device)
        for cnt, (h, m, cands, labels) in enumerate(loader):
            # a training engine's workspace follows its last batch, which may have been a short one
            step = min(h.shape[0], eng.B_alloc)
            for s0 in range(0, h.shape[0], step):
                _, scores, _ = eng.evaluate(news_scoring, h[s0:s0 + step], m[s0:s0 + step], cands[s0:s0 + step],
                                            labels[s0:s0 + step], acc=acc)
                if collect is not None:
                    s, o = scores.cpu().numpy(), 0
                    for c, y in zip(cands[s0:s0 + step], labels[s0:s0 + step]):
                        collect.append((s[o:o + len(c)], y))
                        o += len(c)
            n_local += h.shape[0]
            if cnt % log_steps == 0:
                a = acc.cpu().numpy()
                if a[1]:
                    logging.info("[{}] Ed: {}: {}".format(rank, n_local, "\t".join("{:0.2f}".format(x * 100) for x in a[2:] / a[1])))
        loader.join()
        a = acc.cpu().numpy()
        assert int(a[0]) == n_local, (a[0], n_local)
        return a[2:].copy(), n_local, int(a[1])
    from metrics import mrr_score, ndcg_score, roc_auc_score
    scoring_host = news_scoring.cpu().numpy()
    for cnt, (h, m, cands, labels) in enumerate(loader):
        n_local += h.shape[0]
        users = eng.user_vectors(news_scoring, h, m).cpu().numpy()
        for u, c, y in zip(users, cands, labels):
            if collect is not None:
                collect.append((scoring_host[c] @ u, y))
            if y.mean() == 0 or y.mean() == 1:
                continue
            score = scoring_host[c] @ u
            sums += [roc_auc_score(y, score), mrr_score(y, score), ndcg_score(y, score, 5), ndcg_score(y, score, 10)]
            cnt_metric += 1
        if cnt % log_steps == 0 and cnt_metric:
            logging.info("[{}] Ed: {}: {}".format(rank, n_local, "\t".join("{:0.2f}".format(x * 100) for x in sums / cnt_metric)))
    loader.join()
    return sums, n_local, cnt_metric


def _reduce_metrics(sums, n_local, size, extra=()):
    """test mode's scalar all-reduce (hvd.allreduce(Sum), run.py:372-376): [samples, the four sums, extra...] over the ranks, as
    float64 on the host - every rank gets the same numbers."""
    tot = torch.tensor([float(n_local)] + list(sums) + [float(x) for x in extra], dtype=torch.float64, device="cuda")
    if size > 1:
        torch.distributed.all_reduce(tot)
    return tot.cpu().numpy()


def recommend(args):
    """--mode recommend: of ALL news of --test_data_dir, the --top_k each behaviours line's user should see (the serving step the
    reference stops short of: its test mode scores only the candidates an impression lists).  The checkpoint is loaded as test()
    loads it; one line per behaviours line, in file order: impression_id \\t user_id \\t nid:score ... best first."""
    from dataloader import DataLoaderRecommend
    size, rank, local = utils.init_hvd_cuda(args.enable_hvd, args.enable_gpu)
    ckpt_path = utils.get_checkpoint(args.model_dir, args.load_ckpt_name) if args.load_ckpt_name else utils.latest_checkpoint(args.model_dir)
    assert ckpt_path is not None, "No ckpt found"
    ckpt = torch.load(ckpt_path, map_location="cpu")
    if getattr(args, "use_ema", False):
        if "ema_state_dict" not in ckpt:
            raise KeyError(f"--use_ema True: {ckpt_path} holds no ema_state_dict (it was not trained with --ema_decay)")
        sd = ckpt["ema_state_dict"]
    else:
        sd = ckpt["model_state_dict"]
    eng = _forward_engine(args, args.num_student_layers, sd)
    logging.info(f"Model loaded from {ckpt_path}" + (" (the EMA of the weights)" if getattr(args, "use_ema", False) else ""))
    news_index, news_combined = _news_table(args, args.test_data_dir, "test")
    news_scoring = eng.encode_news(torch.from_numpy(news_combined).cuda())
    logging.info("news scoring num: {}".format(news_scoring.shape[0]))
    nid_of = [None] * news_scoring.shape[0]                      # row -> the table's string id (row 0 is the padding news)
    for nid, row in news_index.items():
        nid_of[row] = nid
    k = args.top_k
    out_path = args.recommend_out or os.path.join(args.model_dir, "recommend.tsv")
    if size > 1:
        out_path = "%s.%d" % (out_path, rank)
    loader = DataLoaderRecommend(news_index=news_index, data_dir=args.test_data_dir, filename_pat=args.filename_pat, args=args,
                                 world_size=size, worker_rank=rank, cuda_device_idx=local, enable_prefetch=True,
                                 enable_shuffle=False, enable_gpu=True)
    n_local, t0 = 0, time.time()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        for cnt, (h, m, _, _, iids, uids) in enumerate(loader):
            idx, score = eng.recommend(news_scoring, h, m, k, exclude_history=args.exclude_history)
            idx, score = idx.cpu().numpy(), score.cpu().numpy()
            for iid, uid, ii, ss in zip(iids, uids, idx, score):
                f.write("%s\t%s\t%s\n" % (iid, uid, " ".join("%s:%.6g" % (nid_of[i], s) for i, s in zip(ii, ss) if i >= 0)))
            n_local += h.shape[0]
            if cnt % args.log_steps == 0:
                logging.info("[{}] Ed: {}: top-{} of {} news, {:.1f} users/s".format(rank, n_local, k, news_scoring.shape[0] - 1,
                                                                                   n_local / max(time.time() - t0, 1e-9)))
    loader.join()
    logging.info("[{}] local_sample_num: {}, {:.1f} users/s, written to {}".format(rank, n_local, n_local / max(time.time() - t0, 1e-9),
                                                                                 out_path))
    return out_path, n_local


if __name__ == "__main__":
    utils.setuplogger()
    args = parse_args()
    {"train": train, "test": test, "get_teacher_emb": get_teacher_emb, "recommend": recommend}[args.mode](args)
    if torch.distributed.is_initialized():
        torch.distributed.destroy_process_group()
