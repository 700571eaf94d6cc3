"""Flag surface of the reference's run.py (Tiny-NewsRec/parameters.py:8-115): every flag keeps its name,
type and default so demo.sh command lines work unchanged.  Flags the reference parses but never reads
 are accepted and ignored here too.  Added flags default to the reference behaviour."""
import argparse
import logging

import utils

_B = utils.str2bool

# "name=default" specs grouped by type (Tiny-NewsRec/parameters.py:8-115, same names / defaults)
_INT = """batch_size=32 npratio=4 shuffle_buffer_size=10000 num_workers=4 filter_num=3 log_steps=100 epochs=1
num_words_title=20 num_words_abstract=50 num_words_body=100 user_log_length=50 word_embedding_dim=300 news_dim=64
news_query_vector_dim=200 user_query_vector_dim=200 num_attention_heads=20 save_steps=1000 max_steps_per_epoch=1000000
num_hidden_layers=8 start_epoch=0 num_teacher_layers=12 num_student_layers=4 num_teachers=4"""
_FLOAT = "lr=0.0001 drop_rate=0.2 pretrain_lr=0.00001 temperature=1.0 coef=1.0"
_BOOL = """enable_gpu=1 enable_hvd=1 enable_shuffle=1 freeze_embedding=0 user_log_mask=1 apply_bert=0 do_lower_case=1
use_pretrain_model=0"""
_STR = {"train_data_dir": "../MIND/MINDlarge_train", "test_data_dir": "../MIND/MINDlarge_test",
        "filename_pat": "behaviors_np4_*.tsv", "model_dir": "./model", "glove_embedding_path": "./glove.840B.300d.txt",
        "load_ckpt_name": None, "model_type": "bert", "model_name": "../bert-base-uncased/pytorch_model.bin",
        "config_name": "../bert-base-uncased/config.json", "tokenizer_name": "../bert-base-uncased/vocab.txt",
        "model": None, "pooling": "att", "pretrain_model_path": None, "tensorboard": None}


def _positive_int(s):
    v = int(s)
    if v < 1:
        raise argparse.ArgumentTypeError("must be at least 1, got %s" % s)
    return v


def _flag_table():
    t = [("mode", str, "train", dict(choices=["train", "test", "get_teacher_emb", "recommend"]))]
    t += [(kv.split("=")[0], int, int(kv.split("=")[1])) for kv in _INT.split()]
    t += [(kv.split("=")[0], float, float(kv.split("=")[1])) for kv in _FLOAT.split()]
    t += [(kv.split("=")[0], _B, kv.split("=")[1] == "1") for kv in _BOOL.split()]     # enable_hvd: True = data parallel over RCCL
    t += [(k, str, v) for k, v in _STR.items()]
    t += [("bert_trainable_layer", int, [], dict(nargs="+", choices=list(range(12)))),
          ("teacher_ckpts", str, [], dict(nargs="+")), ("teacher_emb_paths", str, [], dict(nargs="+")),
          # additions (defaults keep the reference behaviour)
          ("train_embeddings", _B, False, dict(help="also fine-tune bert.embeddings.* (word / position / token-type tables and the embedding LayerNorm) at the encoder's learning rate; the reference freezes them (run.py:101-112); needs --bert_trainable_layer")),
          ("max_grad_norm", float, 0.0, dict(help="clip the gradient by its global L2 norm, torch.nn.utils.clip_grad_norm_ semantics (one norm over everything trainable, coef = min(1, max_norm / (norm + 1e-6))), done on the device after the gradient all-reduce; 0 = off (the reference does not clip)")),
          ("weight_decay", float, 0.0, dict(help="decoupled weight decay (torch.optim.AdamW: p *= 1 - lr * weight_decay before the Adam / AMSGrad update; with --optimizer lamb: LAMB's coupled decay instead, weight_decay * w added to the update that the trust ratio scales) of the 2-D weights outside LayerNorm - biases, LayerNorm parameters and pad_doc are exempt; with --train_embeddings the embedding tables decay - inside the fused update; 0 = off (the reference uses Adam without decay)")),
          ("optimizer", str, "adam", dict(choices=["adam", "lamb"], help="lamb: LAMB (You et al., Large Batch Optimization for Deep Learning, Algorithm 2) on the same Adam / AMSGrad moments, inside the fused update: the step of every 2-D weight outside LayerNorm is rescaled by its trust ratio ||w|| / ||update|| (no clamp; biases, LayerNorm parameters and pad_doc take the plain Adam step), for batches in the thousands (--grad_accum_steps x --batch_size x workers). --weight_decay then means LAMB's COUPLED decay - weight_decay * w is added to the update before the trust ratio scales it - not AdamW's p *= 1 - lr * weight_decay. No new optimiser state: --save_optimizer / --resume work as with adam. The trust ratios (min / median / max) are logged every --log_steps; adam = off (the reference's optimiser)")),
          ("warmup_steps", int, 0, dict(help="multiply every learning rate by u / warmup_steps over the first warmup_steps updates (u = updates taken so far: the first update has rate 0; steps skipped for an fp16 overflow do not count); 0 = no warmup (the reference's rate is constant). The schedule's position is optimiser state: --save_optimizer True writes it into the epoch checkpoint with the Adam moments, and --resume True continues from it (without them a restarted run ramps again from rate 0)")),
          ("lr_decay_steps", int, 0, dict(help="after the warmup, decay every learning rate linearly to 0 at update lr_decay_steps (transformers' get_linear_schedule_with_warmup with num_training_steps = lr_decay_steps), 0 from there on; 0 = constant after the warmup (the reference's rate is constant). The position is saved by --save_optimizer True and restored by --resume True, like the Adam moments")),
          ("ema_decay", float, 0.0, dict(help="keep an exponential moving average of the trainable parameters, ema = ema_decay * ema + (1 - ema_decay) * p after every update (torch.optim.swa_utils.AveragedModel with get_ema_multi_avg_fn), inside the fused update; steps skipped for an fp16 overflow do not advance it. The epoch checkpoint then also holds ema_state_dict (same keys as model_state_dict) and ema (decay, warmup, updates), and --load_ckpt_name resumes the average from it; 0 = off (the reference keeps no average)")),
          ("ema_warmup", _B, False, dict(help="with --ema_decay: use min(ema_decay, (1 + u) / (10 + u)) at the update that u updates precede (TensorFlow's ExponentialMovingAverage num_updates rule), so that a short run's average is not dominated by its starting point. The position follows the updates taken; --save_optimizer True saves it and --resume True restores it, like the Adam moments")),
          ("use_ema", _B, False, dict(help="--mode test: evaluate the averaged parameters (the checkpoint's ema_state_dict, written by a --ema_decay run) instead of model_state_dict; an error if the checkpoint holds none")),
          ("top_k", _positive_int, 10, dict(help="--mode recommend: news per user, 1..128 (the fused score-and-select kernel's limit)")),
          ("recommend_out", str, None, dict(help="--mode recommend: the output file, one line per behaviours line in file order, `impression_id \\t user_id \\t nid:score nid:score ...` best first; with more than one rank, rank r writes PATH.r for its shard; default <model_dir>/recommend.tsv")),
          ("exclude_history", _B, True, dict(help="--mode recommend: never recommend a news the user's history already holds")),
          ("device_metrics", _B, False, dict(help="--mode test: score each impression's candidates and compute AUC / MRR / nDCG@5 / nDCG@10 on the device (one kernel call per batch, totals kept in double in a fixed order, no host copy of the news vectors) instead of the reference's per-impression numpy loop; the same skip rule, tie rule and log lines; the scores are the kernel's own fp32 fma chains, so near-ties may rank differently from the host's BLAS dot products; off = the reference's host loop")),
          ("valid_data_dir", str, None, dict(help="--mode train: a directory laid out like --test_data_dir (news.tsv + behaviours files) to validate on: at the end of every epoch, before the checkpoint is written, and every --valid_steps batches, its news are encoded by the live student and its impressions ranked on the device (the --device_metrics path, sharded over the workers and all-reduced as --mode test does). The four metrics are logged, the epoch checkpoint gains `valid`, and whenever AUC improves on the run's best <model_dir>/best.pt is written (the model keys and `valid`, no optimiser state). Training itself computes the same bits with or without it; unset = off (the reference has no validation)")),
          ("valid_steps", int, 0, dict(help="with --valid_data_dir: also validate after every batch whose 1-based count in the epoch is a multiple of this; must be a multiple of --grad_accum_steps, so that validation never falls inside an accumulation window; 0 = at epoch ends only")),
          ("valid_filename_pat", str, "behaviors_*.tsv", dict(help="with --valid_data_dir: the behaviours files to validate on")),
          ("grad_accum_steps", _positive_int, 1, dict(help="gradient accumulation: one optimiser update per grad_accum_steps batches of --batch_size, on the mean of their gradients (summed on the device in fp32), i.e. an effective batch of grad_accum_steps * batch_size * world impressions; --warmup_steps, --lr_decay_steps and --ema_warmup count updates, not batches; under data parallelism one gradient all-reduce per update, started in the window's last backward (DistributedDataParallel's no_sync for the others); a partial window at the end of an epoch is dropped; an fp16 overflow in any of the batches skips the whole update; 1 = off (the reference updates after every batch)")),
          ("save_optimizer", _B, False, dict(help="the epoch checkpoint also holds optimizer_state_dict (Adam's moments per trainable key, the updates taken - the position of --warmup_steps / --lr_decay_steps / --ema_warmup -, the fp16 loss scaler, the average's update count, the dropout call counter: 12 bytes per trainable element) and train_state (epoch, updates, the flags it ran with); off = the reference's checkpoint keys")),
          ("resume", _B, False, dict(help="with --load_ckpt_name: continue the run that wrote that checkpoint with --save_optimizer True - the optimiser state is restored after the parameters (and the average), the epoch loop and the file-fed loader's shard / shuffle seeds go on at the saved epoch - bit for bit what the uninterrupted run computes; flags that differ from the saved ones are logged as a warning. Off, --load_ckpt_name restores the parameters (and the average) only and --start_epoch is what it was")),
          ("resident_tables", _B, True, dict(help="keep news_combined / teacher tables in HBM and ship indices only")),
          ("cache_frozen_layers", _B, True, dict(help="resident mode: compute the frozen lower encoder layers once per news instead of every step (identical results)")),
          ("dedup_news", _B, True, dict(help="encode each distinct news of a batch once (with and without --resident_tables, the same plan and the same bits in both; identical losses and scores; the gradients are then summed per distinct news first, so a training run agrees with --dedup_news False to rounding, not bit for bit)")),
          ("inbatch_negatives", _B, False, dict(help="--mode train: the target loss ranks each impression's positive against the other impressions' candidates of the batch as well as its own npratio negatives (the distillation and embedding terms keep the impression's own candidates). A foreign candidate slot counts for an impression iff (1) it belongs to another impression, (2) it is not the padding news, (3) no earlier slot of the batch holds the same news - a distinct news counts once, at its first slot -, (4) the news is not among the impression's own candidates, (5) the news is not in the impression's click history. The logged target loss (and train_loss) is then over that larger set and not comparable with a run without the flag; the mean number of such negatives per impression is logged every --log_steps. Under data parallelism each worker uses the candidates of its own batch only (no collective is added). Off = the reference's loss")),
          ("decode_process", _B, True, dict(help="resident mode: TSV decode + de-duplication plan in a child process, so that the decoder does not share the GIL with the thread that launches the kernels (identical batches)")),
          ("dtype", str, "fp16", dict(choices=["bf16", "fp16"], help="16-bit activation type of the HIP kernels (fp16 meets the 1e-3 logit / loss tolerance, bf16 does not: DESIGN.md section 2)")),
          ("allow_random_init", _B, False, dict(help="start from the construction-time initialisation when --model_name does not exist (the reference's from_pretrained raises; so does this build unless this flag or --synthetic is set)")),
          ("synthetic", _B, False, dict(help="random-init weights + synthetic MIND-shaped data (no files needed)"))]
    return t


_FLAGS = _flag_table()


def build_parser():
    ap = argparse.ArgumentParser()
    for f in _FLAGS:
        kw = dict(f[3]) if len(f) > 3 else {}
        if f[0] == "freeze_embedding":
            kw["help"] = "parsed and ignored, exactly as in the reference (nothing reads it there); the embeddings are frozen unless --train_embeddings True"
        ap.add_argument("--" + f[0], type=f[1], default=f[2], **kw)
    return ap


def check_args(args):
    """Flag combinations that cannot run, refused before anything is built."""
    if getattr(args, "resume", False) and not getattr(args, "load_ckpt_name", None):
        raise ValueError("--resume True needs --load_ckpt_name (the checkpoint a --save_optimizer True run wrote)")
    valid_steps = getattr(args, "valid_steps", 0) or 0
    if valid_steps < 0:
        raise ValueError("--valid_steps must be 0 (epoch ends only) or positive, got %d" % valid_steps)
    if valid_steps and not getattr(args, "valid_data_dir", None):
        raise ValueError("--valid_steps %d needs --valid_data_dir (the held-out set to validate on)" % valid_steps)
    accum = getattr(args, "grad_accum_steps", 1) or 1
    if valid_steps % accum:
        raise ValueError("--valid_steps %d is no multiple of --grad_accum_steps %d: validation would fall inside an accumulation "
                         "window" % (valid_steps, accum))


def parse_args(argv=None):
    args = build_parser().parse_args(argv)
    check_args(args)
    logging.info(args)
    return args


if __name__ == "__main__":
    print(parse_args())
