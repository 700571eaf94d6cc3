"""Training-step engine: chains the libtnr_hip.so kernels into forward / backward / AMSGrad.

Host-side mirror of the reference's hot loop body (run.py:178-195): Model.forward
(model_bert.py:262-305) -> total_loss.backward() -> optimizer.step(), for one worker's batch.
torch is used for device memory, streams and (in dist.py) the RCCL all-reduce only; every
arithmetic op on the path is a HIP kernel behind the C ABI, and there is no fallback.

Memory plan (sized for 288 GB HBM3E): parameters live in two flat fp32 buffers (trainable /
frozen) whose slices ARE the nn.Parameters of model_bert.py, gradients and AMSGrad state are flat
buffers of the trainable size, bf16 (and transposed bf16) weight copies are refreshed by one
kernel after each update, activations of the trainable layers stay resident for backward.
"""
import logging
import math
import struct
from types import SimpleNamespace

import numpy as np
import torch

import optstate
import tnr_hip as T

PFX = "student.news_encoder."
BERT = PFX + "bert_model.bert."
QPAD = 256          # news pooling query dim (200) padded to the GEMM tile
AP_LONG = 64        # sequences longer than this take the chunked pooling kernels (tnr_attpool_*_long); a rule of L alone


def _rup(x, m):
    return (x + m - 1) // m * m


def _from(buf, r):
    """Rows r onwards of a workspace buffer (a part's rows: its kernels take their row count as an argument)."""
    return buf[r:] if r else buf


def _fork_join(side, first, second):
    """first(), then second(); with a stream `side`: first() on it beside second() on the current stream, joined behind."""
    if side is None:
        first()
        second()
        return
    main = torch.cuda.current_stream(side.device)
    side.wait_stream(main)
    with torch.cuda.stream(side):
        first()
    second()
    main.wait_stream(side)


class EngineConfig:
    def __init__(self, n_layers=4, trainable_layers=(2, 3), hidden=768, heads=12, inter=3072, news_dim=256,
                 news_query=200, user_query=200, num_teachers=4, user_log_length=50, npratio=4, num_words=30,
                 user_log_mask=False, temperature=1.0, coef=0.2, vocab=30522, max_pos=512, type_vocab=2,
                 ln_eps=1e-12, stage1=False, pooling="att", nrms_heads=0, pos_pad_id=None, train_embeddings=False):
        """stage1=True: the DistillModel of Post-train_KD.ipynb (no user encoders: parameters are
        student.news_encoder.* and transform_matrix.* only; user_log_length is 0, npratio+1 titles per body)."""
        self.stage1 = stage1
        # PLM-NR --model_type (PLM-NR/utils.py:17-21): 'bert' is this encoder with a zero rel-pos table (rel_pos_bias.weight = 0);
        # 'roberta' additionally takes its position rows from the token ids -- cumulative count of non-pad tokens + padding_idx
        # (transformers create_position_ids_from_input_ids) -- with type_vocab 1, max_pos 514 and ln_eps 1e-5 from its config
        self.pos_pad_id = pos_pad_id
        # train_embeddings: bert.embeddings.* (word / position / token-type tables, embedding LayerNorm) join the trainable set.  The
        # reference freezes them with the rest of bert_model (run.py:101-112; its --freeze_embedding flag is read by nothing), so
        # this is an opt-in extension: off, every path and buffer is what it was.  On, the backward runs down through every layer
        # (layers outside trainable_layers pass the gradient on without weight gradients) into tnr_embed_ln_bwd.
        self.train_embeddings = bool(train_embeddings)
        assert not (self.train_embeddings and stage1), \
            "train_embeddings with stage1: the post-training notebooks freeze the embeddings and the joint title/body passes have no embedding backward"
        assert not (self.train_embeddings and pos_pad_id is not None), \
            "train_embeddings with pos_pad_id (roberta): its padding position rows are not covered by the engine's embedding backward"
        assert not self.train_embeddings or len(tuple(trainable_layers)) > 0, \
            "train_embeddings needs at least one trainable encoder layer (the backward starts at the layer loop)"
        # args.pooling (model_bert.py:130-135): 'att' | 'cls' | anything else = mean ; args.model == 'NRMS' puts a
        # nrms_heads x 16 self-attention in front of every user encoder's pooling (model_bert.py:145-148)
        self.pooling = pooling if pooling in ("att", "cls") else "mean"
        self.nrms_heads = int(nrms_heads)
        assert not self.nrms_heads or self.nrms_heads * 16 == news_dim, "NRMS: num_attention_heads * 16 must equal news_dim (scorer bmm)"
        self.n_layers, self.trainable_layers = n_layers, tuple(sorted(trainable_layers))
        self.H, self.A, self.I, self.D = hidden, heads, inter, news_dim
        self.Qn, self.Qu, self.T = news_query, user_query, num_teachers
        self.U, self.C, self.L = user_log_length, npratio + 1, num_words
        self.user_log_mask, self.temperature, self.coef = bool(user_log_mask), float(temperature), float(coef)
        self.vocab, self.max_pos, self.type_vocab, self.ln_eps = vocab, max_pos, type_vocab, ln_eps
        assert hidden == heads * 64, "attention kernel is built for head size 64"
        assert hidden % 256 == 0 and inter % 128 == 0 and news_dim % 4 == 0 and news_query <= QPAD
        assert 1 <= num_words <= 512, "attention kernels cover sequences of up to 512 tokens"
        assert all(0 <= l < n_layers for l in self.trainable_layers)


NRMS_W = ["multi_head_self_attn.W_%s.weight" % n for n in "QKV"]      # stacked [W_Q; W_K; W_V] (3D, D) per encoder
NRMS_B = ["multi_head_self_attn.W_%s.bias" % n for n in "QKV"]


def layer_param_order(l):
    p = BERT + "encoder.layer.%d." % l
    return [p + "attention.self.query.weight", p + "attention.self.key.weight", p + "attention.self.value.weight",
            p + "attention.self.query.bias", p + "attention.self.key.bias", p + "attention.self.value.bias",
            p + "attention.output.dense.weight", p + "attention.output.dense.bias",
            p + "attention.output.LayerNorm.weight", p + "attention.output.LayerNorm.bias",
            p + "intermediate.dense.weight", p + "intermediate.dense.bias",
            p + "output.dense.weight", p + "output.dense.bias",
            p + "output.LayerNorm.weight", p + "output.LayerNorm.bias"]


def param_shapes(cfg):
    """state_dict schema of model_bert.Model, in the engine's storage order."""
    H, I, D, T_ = cfg.H, cfg.I, cfg.D, cfg.T
    s = {}
    if cfg.nrms_heads and not cfg.stage1:
        for i in range(T_):
            for n in NRMS_W:
                s["teachers.%d.%s" % (i, n)] = (D, D)
        for i in range(T_):
            for n in NRMS_B:
                s["teachers.%d.%s" % (i, n)] = (D,)
    for i in range(0 if cfg.stage1 else T_):
        s["teachers.%d.attn.att_fc1.weight" % i] = (cfg.Qu, D)
    for i in range(0 if cfg.stage1 else T_):
        s["teachers.%d.attn.att_fc1.bias" % i] = (cfg.Qu,)
    for i in range(0 if cfg.stage1 else T_):
        s["teachers.%d.attn.att_fc2.weight" % i] = (1, cfg.Qu)
    for i in range(0 if cfg.stage1 else T_):
        s["teachers.%d.pad_doc" % i] = (1, D)
    for i in range(0 if cfg.stage1 else T_):
        s["teachers.%d.attn.att_fc2.bias" % i] = (1,)
    s[BERT + "embeddings.word_embeddings.weight"] = (cfg.vocab, H)
    s[BERT + "embeddings.position_embeddings.weight"] = (cfg.max_pos, H)
    s[BERT + "embeddings.token_type_embeddings.weight"] = (cfg.type_vocab, H)
    s[BERT + "embeddings.LayerNorm.weight"] = (H,)
    s[BERT + "embeddings.LayerNorm.bias"] = (H,)
    for l in range(cfg.n_layers):
        for k in layer_param_order(l):
            if k.endswith("intermediate.dense.weight"):
                s[k] = (I, H)
            elif k.endswith("intermediate.dense.bias"):
                s[k] = (I,)
            elif k.endswith(".output.dense.weight") and "attention" not in k:
                s[k] = (H, I)
            elif k.endswith("weight") and "LayerNorm" not in k:
                s[k] = (H, H)
            else:
                s[k] = (H,)
    s[BERT + "pooler.dense.weight"] = (H, H)
    s[BERT + "pooler.dense.bias"] = (H,)
    s[BERT + "rel_pos_bias.weight"] = (cfg.A, 32)
    s[PFX + "bert_model.classifier.weight"] = (2, H)
    s[PFX + "bert_model.classifier.bias"] = (2,)
    # heads: order = order in which their gradients complete / are laid out by the kernels
    if cfg.pooling == "att":
        s[PFX + "attn.att_fc1.weight"] = (cfg.Qn, H)
        s[PFX + "attn.att_fc1.bias"] = (cfg.Qn,)
        s[PFX + "attn.att_fc2.weight"] = (1, cfg.Qn)
        s[PFX + "attn.att_fc2.bias"] = (1,)
    s[PFX + "dense.weight"] = (D, H)
    s[PFX + "dense.bias"] = (D,)
    if cfg.nrms_heads and not cfg.stage1:
        for n in NRMS_W:
            s["student.user_encoder." + n] = (D, D)
        for n in NRMS_B:
            s["student.user_encoder." + n] = (D,)
    if not cfg.stage1:
        s["student.user_encoder.attn.att_fc1.weight"] = (cfg.Qu, D)
        s["student.user_encoder.attn.att_fc1.bias"] = (cfg.Qu,)
        s["student.user_encoder.attn.att_fc2.weight"] = (1, cfg.Qu)
        s["student.user_encoder.pad_doc"] = (1, D)
        s["student.user_encoder.attn.att_fc2.bias"] = (1,)
    for i in range(T_):
        s["transform_matrix.%d.weight" % i] = (D, D)
    for i in range(T_):
        s["transform_matrix.%d.bias" % i] = (D,)
    return s


def is_trainable(cfg, name):
    """run.py:101-112: teachers frozen; bert_model frozen except encoder.layer[i], i in trainable_layers (and, an extension the
    reference does not have, bert.embeddings.* under cfg.train_embeddings; rel_pos_bias, pooler and classifier stay frozen)."""
    if name.startswith("teachers."):
        return False
    if name.startswith(PFX + "bert_model."):
        if getattr(cfg, "train_embeddings", False) and name.startswith(BERT + "embeddings."):
            return True
        for l in cfg.trainable_layers:
            if name.startswith(BERT + "encoder.layer.%d." % l):
                return True
        return False
    return True


class _ReduceBatch:
    """Fixed-order partial-sum reductions of one gradient bucket, done by ONE tnr_reduce_multi launch.
    The job list is static (same buffers every step): recorded during the first backward, then replayed."""

    def __init__(self, dev):
        self.dev, self.jobs, self.table = dev, [], None

    def add(self, part, rows, stride, n, out, accumulate=0, scale=1.0):
        """out (+)= scale * column sums of part ; the scale rides in the upper half of the descriptor's last word."""
        if self.table is None:
            sb = 0 if scale == 1.0 else struct.unpack("<I", struct.pack("<f", scale))[0]
            self.jobs.append((part.data_ptr(), rows, stride, n, out.data_ptr(), int(accumulate) | (sb << 32)))

    def flush(self):
        if not self.jobs:
            return
        if self.table is None:
            l1, l2 = [], []
            for part, rows, stride, n, out, acc in self.jobs:
                chunks = max(1, min(rows // 32, 16))                 # row chunks summed in place first (tall partials)
                per = (rows + chunks - 1) // chunks
                chunks = (rows + per - 1) // per
                for c0 in range(0, n, 64):
                    nc = min(64, n - c0)
                    if chunks > 1:
                        for ch in range(chunks):
                            r0 = ch * per
                            src = part + 4 * (r0 * stride + c0)
                            l1.append((src, min(per, rows - r0), stride, nc, src, 0))
                        l2.append((part + 4 * c0, chunks, per * stride, nc, out + 4 * c0, acc))
                    else:
                        l2.append((part + 4 * c0, rows, stride, nc, out + 4 * c0, acc))
            mk = lambda rows_: (torch.tensor(rows_, dtype=torch.int64, device=self.dev), len(rows_)) if rows_ else None
            self.table = (mk(l1), mk(l2))
        for t in self.table:
            if t is not None:
                T.call("tnr_reduce_multi", t[0], t[1])


def pack_impressions(cands, labels):
    """The eval loader's per-impression arrays as tnr_rank_metrics takes them -> (cand int32, label int32, offs int32 (B + 1)):
    impression b owns [offs[b], offs[b + 1]) of cand and label.  Host only.  Refused: a label other than 0 or 1, a negative
    candidate index, unlike lengths, more candidates than int32 offsets hold."""
    n = len(cands)
    if len(labels) != n:
        raise ValueError("pack_impressions: %d candidate arrays, %d label arrays" % (n, len(labels)))
    cs = [np.asarray(c).reshape(-1) for c in cands]
    ys = [np.asarray(y).reshape(-1) for y in labels]
    for b, (c, y) in enumerate(zip(cs, ys)):
        if c.size != y.size:
            raise ValueError("pack_impressions: impression %d has %d candidates and %d labels" % (b, c.size, y.size))
    offs = np.zeros(n + 1, np.int64)
    np.cumsum([c.size for c in cs], out=offs[1:])
    if offs[-1] >= 2 ** 31:
        raise ValueError("pack_impressions: %d candidates do not fit int32 offsets" % offs[-1])
    cand = np.concatenate(cs) if offs[-1] else np.zeros(0, np.int64)
    label = np.concatenate(ys) if offs[-1] else np.zeros(0, np.int64)
    if cand.size and (cand.min() < 0 or cand.max() >= 2 ** 31):
        raise ValueError("pack_impressions: candidate index %d outside [0, 2^31)" % (cand.min() if cand.min() < 0 else cand.max()))
    if not ((label == 0) | (label == 1)).all():
        raise ValueError("pack_impressions: labels must be 0 or 1, found %s" % label[(label != 0) & (label != 1)][0])
    return cand.astype(np.int32), label.astype(np.int32), offs.astype(np.int32)


def lr_schedule(u, warmup_steps=0, lr_decay_steps=0):
    """Multiplier of every learning rate at an update that `u` updates precede (step(warmup_steps=W, lr_decay_steps=T)):
    u / W while u < W (the first update has rate 0), then max(0, (T - u) / max(1, T - W)) if T > 0 and 1 if T == 0 -
    transformers' get_linear_schedule_with_warmup / get_constant_schedule_with_warmup as LambdaLR applies them.  W = T = 0: 1."""
    u, W, T_ = int(u), int(warmup_steps or 0), int(lr_decay_steps or 0)
    if u < W:
        return u / W
    if T_ > 0:
        return max(0.0, (T_ - u) / max(1, T_ - W))
    return 1.0


def ema_decay_at(u, decay, warmup=False):
    """Decay of the parameter average at an update that `u` updates precede (step(ema_decay=decay, ema_warmup=warmup)):
    `decay`, or with warmup min(decay, (1 + u) / (10 + u)) - TF's ExponentialMovingAverage(num_updates=u) rule: the first updates
    weigh in heavily (0.1, 0.18, 0.25, ...), so the average leaves its starting point as fast as the parameters do."""
    u, decay = int(u), float(decay)
    return min(decay, (1.0 + u) / (10.0 + u)) if warmup else decay


def decays(name, shape):
    """The decay set of step(weight_decay=...): 2-D `.weight`s outside LayerNorm (Linear and embedding matrices); biases, every
    LayerNorm parameter and pad_doc are exempt."""
    return name.endswith(".weight") and len(shape) == 2 and "LayerNorm" not in name


def decay_words(slot, n_train):
    """One bit per element of the flat trainable buffer (element e = bit e & 31 of word e >> 5, uint32), set for the elements of
    the parameters that decay; alignment gaps and reserved rows stay clear.  A pure host function of the slot table."""
    bits = np.zeros(_rup(n_train, 32), dtype=bool)
    for name, (tr, o, n, shp) in slot.items():
        if tr and decays(name, shp):
            bits[o:o + n] = True
    return np.packbits(bits.reshape(-1, 32), axis=1, bitorder="little").view("<u4").reshape(-1).copy()


LAMB_CHUNK = 4096       # elements per chunk at most (csrc/lamb.hip: one workgroup of 256 lanes x 4 x 16 bytes)


def lamb_chunks(slot, n_train):
    """The element-to-tensor map of step(lamb=True), a pure host function of the slot table like decay_words:
    (names, chunks, tensors).  names: the trainable tensors in the order of their offsets; the index is the tensor id.
    chunks: int32 (n_chunks, 4) rows (first element, count, tensor id, flags), flags bit 0 = decays(name, shape) (the adapted
    set).  A chunk never crosses its tensor's end and holds 1 .. LAMB_CHUNK elements; inside a tensor chunks end at absolute
    multiples of LAMB_CHUNK, so that only a tensor's first chunk can start off a 16-byte boundary.  Together they cover every
    element of every trainable tensor exactly once and nothing else: alignment gaps and reserved rows belong to no chunk.
    tensors: int32 (n_tensors, 4) rows (first chunk, number of chunks, adapted, 0); a tensor's chunks are consecutive."""
    names = sorted((k for k, s in slot.items() if s[0] and s[2] > 0), key=lambda k: slot[k][1])
    chunks, tensors = [], []
    for t, name in enumerate(names):
        _, o, n, shp = slot[name]
        assert 0 <= o and o + n <= n_train, name
        flag = 1 if decays(name, shp) else 0
        first_chunk, pos = len(chunks), o
        while pos < o + n:
            end = min(o + n, (pos // LAMB_CHUNK + 1) * LAMB_CHUNK)
            chunks.append((pos, end - pos, t, flag))
            pos = end
        tensors.append((first_chunk, len(chunks) - first_chunk, flag, 0))
    return (names, np.asarray(chunks, dtype=np.int32).reshape(-1, 4), np.asarray(tensors, dtype=np.int32).reshape(-1, 4))


LOSS_SCALE = 1024.0     # static scale of the 16-bit backward in fp16 mode (gradients of ~1e-6 would underflow); it enters at
                        # the pooling backward and leaves in the kernels that write parameter gradients (weight-gradient slab
                        # reduce, bias / LayerNorm partial reductions), so flat_g always holds the true gradients


class LossScaler:
    """Dynamic loss scale of the fp16 build (host side; the device side is tnr_grad_nonfinite + tnr_amsgrad_step_guarded).
    The reference trains in fp32 (run.py:134,194-195) and has no such thing; with 16-bit activation gradients ONE overflow would
    put inf / nan into m, v and - for good - vmax.  Every optimiser step gets a stamp; a kernel looks for non-finite values in
    the (reduced) flat gradient and records the stamp in `guard`, and the update kernels of that stamp do nothing: the step is
    skipped on the device without the host knowing.  The host reads guard back asynchronously and looks at the answer TWO steps
    later (the GPU is never drained for it): an overflow halves the multiplier `mult` (the engine's scale is base x mult) and takes
    the skipped step out of Adam's step count; `growth_interval` clean steps in a row double it again, up to `max_mult`.
    bf16 has fp32's exponent range: scaler disabled, nothing launched."""

    def __init__(self, dev, enabled, growth_interval=2000, max_mult=64.0, min_mult=2.0 ** -20):
        self.enabled = bool(enabled) and torch.device(dev).type == "cuda"
        self.mult, self.stamp, self.clean, self.skipped, self.run_of_skips = 1.0, 0, 0, 0, 0
        self.growth_interval, self.max_mult, self.min_mult = growth_interval, max_mult, min_mult
        self.guard = torch.zeros(4, dtype=torch.int32, device=dev) if self.enabled else None
        self.pending = []                    # (stamp, pinned host word, event, multiplier that step's backward ran with) in issue order
        self._ring = torch.zeros(8, dtype=torch.int32).pin_memory() if self.enabled else None    # at most lag + 1 answers are outstanding

    def poll(self, eng, lag=2):
        """Answers of the steps at least `lag` stamps back.  Deterministic (which answers are used depends on the step number
        only, never on timing: data-parallel ranks must change their scale and step count at the same step); the event of a step
        two back has normally long completed - a host running further ahead than that waits here, with a full step still queued.
        An answer arrives two steps late, so the two backwards after an overflow have already run at the old scale and
        overflow with it: an overflow takes the multiplier to HALF OF WHAT THAT STEP'S BACKWARD RAN WITH, if it is not below
        that already - one cause, one halving; the later two steps are still skipped on the device and still leave Adam's
        count."""
        while self.pending and self.pending[0][0] <= self.stamp - lag + 1:
            stamp, host, ev, used = self.pending.pop(0)
            ev.synchronize()
            if int(host[0]) == stamp:        # that step found inf / nan: it was skipped on the device
                self.skipped += 1
                self.clean = 0
                self.run_of_skips += 1
                self.mult = max(min(self.mult, used * 0.5), self.min_mult)
                eng.step_count = max(eng.step_count - 1, 0)
                if self.run_of_skips == 16:  # a smaller scale cures a backward overflow within a few steps, never a forward one
                    logging.warning("16 optimiser steps in a row skipped for inf / nan gradients although the loss scale went down "
                                    "to %g: the fp16 FORWARD overflows (or the data holds inf / nan) - use --dtype bf16", eng.gscale)
            else:
                self.run_of_skips = 0
                self.clean += 1
                if self.clean >= self.growth_interval and self.mult < self.max_mult:
                    self.mult, self.clean = self.mult * 2.0, 0

    def record(self, used):
        """`used`: the multiplier this step's backward ran with (Engine.step reads it before poll may change it)."""
        host = self._ring[self.stamp % 8: self.stamp % 8 + 1]
        host.copy_(self.guard[:1], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self.pending.append((self.stamp, host, ev, used))

    def drain(self, eng):
        """Wait for every outstanding answer (end of an epoch / before a checkpoint / tests)."""
        self.poll(eng, lag=0)

    def reset(self, eng):
        """New weights (load_state_dict) or a new benchmark leg: outstanding answers are consumed, then the scale starts over;
        skipped-step totals stay (they are a log figure)."""
        self.drain(eng)
        self.mult, self.clean, self.run_of_skips = 1.0, 0, 0


class Engine:
    def __init__(self, cfg, device="cuda:0", max_batch=32, dtype="fp16", share=None, extra_rows=0, extra_seqs=0):
        """extra_rows / extra_seqs: room for that many more token rows / sequences behind this engine's own in every per-token /
        per-sequence workspace (stage 1's joint passes: the body pass's rows directly behind the title pass's, stage1.py).
        dtype: 16-bit activation / weight-copy type, "fp16" (default: meets the 1e-3 logit / loss bound) or "bf16".
        fp16 has the same MFMA rate and 3 more mantissa bits; its backward runs on activation gradients scaled by LOSS_SCALE from the
        pooling backward down (everything 16-bit); the kernels that write parameter gradients multiply by 1 / LOSS_SCALE (exact)."""
        T.lib()                      # fail loudly if the HIP library is missing
        assert dtype in ("bf16", "fp16")
        self.f16 = dtype == "fp16"
        self.dtype = dtype
        self.tdt = torch.float16 if self.f16 else torch.bfloat16
        self._gbase = LOSS_SCALE if self.f16 else 1.0
        self.cfg, self.dev = cfg, torch.device(device)
        self.lnames = [layer_param_order(l) for l in range(cfg.n_layers)]     # formatted once: the layer blocks of every step look them up
        # dynamic loss scale (fp16 only); engines that share parameters share it (stage 1: both passes of a step use one scale)
        self.scaler = share.scaler if share is not None else LossScaler(self.dev, self.f16)
        self.step_count = 0
        self._n_alloc = 0
        self._topk_ws = {}           # topk's workspace, by size: allocated by the first call, never by training
        if share is None:
            self._build_params()
            self._build_shadows()
        else:
            # a second pass over the SAME model at another sequence length (stage 1: titles and bodies): parameters,
            # gradients, optimiser state and 16-bit weight copies are the other engine's, workspaces are its own
            for k in ("shapes", "slot", "n_train", "n_frozen", "flat", "flat_g", "adam_m", "adam_v", "adam_vmax", "params",
                      "grads", "lo", "sh", "sh_a1", "sh_a1T", "b_a1", "desc_all", "desc_train"):
                setattr(self, k, getattr(share, k))
        # global-norm gradient clipping (step(max_grad_norm=...)): buffers come with the first clipped step and belong to the engine
        # that owns flat_g; never requested, nothing is allocated
        self._clip_owner = self if share is None else share._clip_owner
        self._clip_state = None
        self._decay_map = None       # step(weight_decay > 0): the owner's decay bits on the device, made on first use
        self.lr_scale = None         # the host's multiplier of the last step's learning rates while a schedule is on, else None
        self._ema = None             # step(ema_decay > 0): the owner's average of flat[True], made on first use
        self._lamb_state = None      # step(lamb=True): the owner's chunk / tensor / trust tables and partial buffer, made on first use
        self._ema_updates = [0, 0]   # updates counted into it, and the scaler's skipped-step total that count already reflects
        self._acc = None             # backward(micro=(j, K > 1)): the owner's accumulator of flat_g over a window, made on first use
        self._acc_held = 0           # micro-gradients the owner's accumulator holds (0 outside an accumulation window)
        self.max_batch = max_batch
        self.extra_rows, self.extra_seqs = int(extra_rows), int(extra_seqs)
        self.drop = None             # set_dropout(): train-mode dropout of the stage-0 / stage-1 notebooks
        self.drop_calls = 0
        self._alloc_workspace(max_batch)
        self.comm = None             # set by dist.attach()

    @property
    def gscale(self):
        """Loss scale of the 16-bit backward: LOSS_SCALE x (batch factor) x the dynamic multiplier (powers of two: exact)."""
        return self._gbase * self.scaler.mult

    @property
    def ginv(self):
        return 1.0 / self.gscale

    # ------------------------------------------------------------------ parameters
    def _groups(self):
        """Storage groups: members are contiguous (no padding inside), every group starts 64-float aligned.
        Stacks that kernels read as one array: per-teacher params, q/k/v weights and biases, the student
        user-encoder block (w1, then tnr_user_bwd_pre/post's partial layout [b1|w2|pad|b2]), transform matrices."""
        cfg = self.cfg
        T_ = cfg.T
        tstack = lambda suffix: ["teachers.%d.%s" % (i, suffix) for i in range(T_)]
        groups = []
        if T_ and cfg.nrms_heads and not cfg.stage1:
            groups.append((["teachers.%d.%s" % (i, n) for i in range(T_) for n in NRMS_W], None))
            groups.append((["teachers.%d.%s" % (i, n) for i in range(T_) for n in NRMS_B], None))
        if T_ and not cfg.stage1:
            for suffix in ("attn.att_fc1.weight", "attn.att_fc1.bias", "attn.att_fc2.weight", "pad_doc", "attn.att_fc2.bias"):
                groups.append((tstack(suffix), None))
        for k in ("word_embeddings.weight", "position_embeddings.weight", "token_type_embeddings.weight",
                  "LayerNorm.weight", "LayerNorm.bias"):
            groups.append(([BERT + "embeddings." + k], None))
        for l in range(cfg.n_layers):
            n = layer_param_order(l)
            groups.append((n[0:3], None))
            groups.append((n[3:6], None))
            for k in n[6:]:
                groups.append(([k], None))
        for k in (BERT + "pooler.dense.weight", BERT + "pooler.dense.bias", BERT + "rel_pos_bias.weight",
                  PFX + "bert_model.classifier.weight", PFX + "bert_model.classifier.bias"):
            groups.append(([k], None))
        if cfg.pooling == "att":
            groups.append(([PFX + "attn.att_fc1.weight"], QPAD * cfg.H))     # rows Qn..QPAD stay zero
            groups.append(([PFX + "attn.att_fc1.bias"], QPAD))
            for k in ("attn.att_fc2.weight", "attn.att_fc2.bias"):
                groups.append(([PFX + k], None))
        for k in ("dense.weight", "dense.bias"):
            groups.append(([PFX + k], None))
        ue = "student.user_encoder."
        if cfg.nrms_heads and not cfg.stage1:
            groups.append(([ue + n for n in NRMS_W], None))
            groups.append(([ue + n for n in NRMS_B], None))
        if not cfg.stage1:
            groups.append(([ue + "attn.att_fc1.weight", ue + "attn.att_fc1.bias", ue + "attn.att_fc2.weight", ue + "pad_doc",
                            ue + "attn.att_fc2.bias"], None))
        if T_:
            groups.append((["transform_matrix.%d.weight" % i for i in range(T_)], None))
            groups.append((["transform_matrix.%d.bias" % i for i in range(T_)], None))
        return groups

    def _build_params(self):
        cfg = self.cfg
        shapes = param_shapes(cfg)
        self.shapes = shapes
        off = {True: 0, False: 0}
        self.slot = {}
        seen = set()
        for names, reserve in self._groups():
            tr = is_trainable(cfg, names[0])
            o = off[tr]
            for name in names:
                shp = shapes[name]
                n = int(math.prod(shp))
                self.slot[name] = (tr, o, n, shp)
                o += n
                seen.add(name)
            off[tr] = _rup(max(o, off[tr] + (reserve or 0)), 64)
        assert seen == set(shapes), set(shapes) ^ seen
        self.n_train, self.n_frozen = max(off[True], 64), max(off[False], 64)
        dev = self.dev
        self.flat = {True: torch.zeros(self.n_train, device=dev), False: torch.zeros(self.n_frozen, device=dev)}
        self.flat_g = torch.zeros(self.n_train, device=dev)
        self.adam_m = torch.zeros(self.n_train, device=dev)
        self.adam_v = torch.zeros(self.n_train, device=dev)
        self.adam_vmax = torch.zeros(self.n_train, device=dev)
        self.params, self.grads = {}, {}
        for name in shapes:
            tr, o, n, shp = self.slot[name]
            self.params[name] = self.flat[tr][o:o + n].view(shp)
            if tr:
                self.grads[name] = self.flat_g[o:o + n].view(shp)

    def _c(self, name, *args):
        """Kernel call; 16-bit entry points take the _f16 variant in fp16 mode."""
        T.call(name + "_f16" if (self.f16 and name in T.TYPED) else name, *args)

    def _q(self, name, *args):
        return T.query(name + "_f16" if (self.f16 and name in T.TYPED) else name, *args)

    def p(self, name):
        return self.params[name]

    def off(self, name):
        return self.slot[name][1]

    def _view(self, first, numel, shape, grad=False):
        tr, o, _, _ = self.slot[first]
        buf = self.flat_g if grad else self.flat[tr]
        return buf[o:o + numel].view(shape)

    def load_state_dict(self, sd):
        """sd: {key: array-like fp32}; every key of the reference schema must be present."""
        missing = [k for k in self.shapes if k not in sd]
        if missing:
            raise KeyError("missing keys: %s" % missing[:5])
        for k, shp in self.shapes.items():
            v = sd[k]
            v = v if isinstance(v, torch.Tensor) else torch.as_tensor(v)
            if tuple(v.shape) != tuple(shp):
                raise ValueError("%s: shape %s != %s" % (k, tuple(v.shape), shp))
            self.params[k].copy_(v.to(self.dev, torch.float32))
        self.refresh_shadows(all_layers=True)
        if self.scaler.enabled:              # answers still outstanding belong to the old weights; the scale starts over
            self.scaler.reset(self)

    def state_dict(self):
        return {k: v.detach().clone() for k, v in self.params.items()}

    # ------------------------------------------------------------------ dropout (train mode of the notebooks)
    def set_dropout(self, p_hidden, p_attn, seed, pass_id=0):
        """hidden_dropout_prob / attention_probs_dropout_prob of the UniLM config (tnlrv3/config/*.json:2,4), live in the
        notebooks because they call .train() (Post-train_KD.ipynb cell 19:6): embeddings (tnlrv3/modeling.py:177), attention
        probabilities (:224), BertSelfOutput / BertOutput (:287, :306).  run.py never calls .train(), so its path has none.
        Counter-based masks (csrc/dropout.h): every encode() is one numbered forward call = 2 * count + pass_id (two engines that
        share parameters -- titles and bodies -- take different pass_ids); backward regenerates the masks from that number.
        p = 0 for both turns dropout off (bit-identical to never having called this)."""
        if (p_hidden or 0.0) <= 0.0 and (p_attn or 0.0) <= 0.0:
            self.drop = None
            return
        assert not self.cfg.train_embeddings, "train_embeddings: the engine's embedding backward takes no dropout site (kernel level only)"
        self.drop = dict(p_hidden=float(p_hidden or 0.0), p_attn=float(p_attn or 0.0), seed=int(seed), pass_id=int(pass_id))
        if self.dyprem is None:
            z = lambda *s_: torch.zeros(s_, device=self.dev, dtype=self.tdt)
            self.dyprem, self.dh1prem = z(self.Mp, self.cfg.H), z(self.Mp, self.cfg.H)

    def _begin_drop_call(self, train=True):
        """Number the forward call that starts now (encode(); Stage1Engine's joint passes call it once per pass)."""
        self.drop_cur = None
        if self.drop is not None and train:
            self.drop_cur = dict(self.drop, call=2 * self.drop_calls + self.drop["pass_id"])
            self.drop_calls += 1

    def _dsite(self, kind, layer):
        """tnr_dropout_t of one site of the CURRENT forward call (None when dropout is off for that kind)."""
        d = self.drop_cur
        if d is None:
            return None
        return T.Dropout.site_of(d["p_attn"] if kind == T.DROP_PROB else d["p_hidden"], d["seed"], kind, layer, d["call"])

    # ------------------------------------------------------------------ bf16 weight copies
    def _build_shadows(self):
        cfg, dev, bf = self.cfg, self.dev, self.tdt
        H, I = cfg.H, cfg.I
        lo = min(cfg.trainable_layers) if cfg.trainable_layers else cfg.n_layers
        if cfg.train_embeddings:
            lo = 0           # the gradient runs down to the embeddings: every layer keeps its activations and has transposed copies
        self.lo = lo
        self.sh = []
        for l in range(cfg.n_layers):
            d = dict(qkv=torch.zeros((3 * H, H), device=dev, dtype=bf), o=torch.zeros((H, H), device=dev, dtype=bf),
                     w1=torch.zeros((I, H), device=dev, dtype=bf), w2=torch.zeros((H, I), device=dev, dtype=bf))
            if l >= lo:      # dgrad needs the transposed copies
                d.update(qkvT=torch.zeros((H, 3 * H), device=dev, dtype=bf), oT=torch.zeros((H, H), device=dev, dtype=bf),
                         w1T=torch.zeros((H, I), device=dev, dtype=bf), w2T=torch.zeros((I, H), device=dev, dtype=bf))
            self.sh.append(d)
        self.sh_a1 = torch.zeros((QPAD, H), device=dev, dtype=bf)
        self.sh_a1T = torch.zeros((H, QPAD), device=dev, dtype=bf)
        self.b_a1 = self._view(PFX + "attn.att_fc1.bias", QPAD, (QPAD,)) if cfg.pooling == "att" else None

        def table(layers, with_heads):
            rows = []
            for l in layers:
                d, names = self.sh[l], layer_param_order(l)
                for i in range(3):
                    rows.append((self.p(names[i]), H, H, d["qkv"][i * H:], H, d["qkvT"][:, i * H:] if "qkvT" in d else None, 3 * H))
                rows.append((self.p(names[6]), H, H, d["o"], H, d.get("oT"), H))
                rows.append((self.p(names[10]), I, H, d["w1"], H, d.get("w1T"), I))
                rows.append((self.p(names[12]), H, I, d["w2"], I, d.get("w2T"), H))
            if with_heads and cfg.pooling == "att":
                rows.append((self.p(PFX + "attn.att_fc1.weight"), cfg.Qn, H, self.sh_a1, H, self.sh_a1T, QPAD))
            desc, start, tot = [], [0], 0
            for src, r, c, dst, ld, dstT, ldT in rows:
                desc.append([src.data_ptr(), r, c, dst.data_ptr(), ld, dstT.data_ptr() if dstT is not None else 0, ldT, 0])
                tot += ((r + 31) // 32) * ((c + 31) // 32)
                start.append(tot)
            return (torch.tensor(desc, dtype=torch.int64, device=dev), len(desc), tot,
                    torch.tensor(start, dtype=torch.int64, device=dev))

        self.desc_all = table(range(cfg.n_layers), True)
        self.desc_train = table(cfg.trainable_layers, True)

    def refresh_shadows(self, all_layers=False):
        d = self.desc_all if all_layers else self.desc_train
        self._c("tnr_refresh_shadows", d[0], d[1], d[2], d[3])
        if all_layers:
            self.fcache = None                 # every weight may have changed: the frozen-prefix cache is stale
            self.refresh_rel()

    def refresh_rel(self):
        """(A, Lr, Lr) additive rel-pos table of this engine's sequence length (depends on a frozen weight only)."""
        T.call("tnr_relpos_table", self.p(BERT + "rel_pos_bias.weight"), self.cfg.A, self.cfg.L, self.rel)
        self._rel_stale = False

    # ------------------------------------------------------------------ workspaces
    def _alloc_workspace(self, B):
        cfg, dev, bf = self.cfg, self.dev, self.tdt
        H, I, D, L = cfg.H, cfg.I, cfg.D, cfg.L
        N = B * (cfg.U + cfg.C)
        Mp = _rup(N * L + self.extra_rows, 128)
        self.B_alloc, self.N_alloc, self.Mp = B, N, Mp
        self._inbatch = None               # the in-batch-negatives buffers follow the batch (_inbatch_buffers)
        Nx = N + self.extra_seqs           # per-sequence partials / pooled vectors with room for a second pass's sequences
        if self.f16:
            # the losses are batch means, so activation gradients shrink as 1 / B: the scale grows with the batch in powers of two
            # beyond the B = 32 it was set for (B = 512 at the fixed scale: parameter gradients 1.8e-3 off the mean of their
            # B = 32 pieces; 1e-6 with it - a power-of-two batch then sees the very 16-bit values its pieces saw;
            # tools/scratch/big_batch.py, test_big_batch_equals_its_pieces).  B <= 32: unchanged.
            k = 0
            while (32 << k) < B and k < 5:
                k += 1
            self._gbase = LOSS_SCALE * (1 << k)
        z = lambda *s, dt=bf: torch.zeros(s, device=dev, dtype=dt)
        f = lambda *s: torch.zeros(s, device=dev, dtype=torch.float32)
        Lr = _rup(L, 32)
        self.Lr = Lr
        self.tok = torch.zeros((N, 2 * L), device=dev, dtype=torch.int64)
        self.nidx_buf = torch.zeros(N, device=dev, dtype=torch.int32)
        self.mask_add = f(N, Lr)
        self.rel = f(cfg.A, Lr, Lr)
        self.lse = f(N, cfg.A, Lr) if L > 32 else None        # long-sequence attention keeps the softmax statistics
        self.delta = f(N, cfg.A, Lr) if L > 32 else None
        self.x0 = z(Mp, H)
        n_keep = cfg.n_layers - self.lo
        mk = lambda: dict(qkv=z(Mp, 3 * H), ctx=z(Mp, H), h1pre=z(Mp, H), st1=f(Mp, 2), h1=z(Mp, H), u=z(Mp, I),
                          g=z(Mp, I), ypre=z(Mp, H), st2=f(Mp, 2), y=z(Mp, H),
                          lse=f(N, cfg.A, Lr) if L > 32 else None)
        self.act = [mk() for _ in range(n_keep)]          # resident activations of layers >= lo
        self.scr = mk() if self.lo > 0 else None           # scratch for frozen layers below lo
        self.scr_y = [z(Mp, H), z(Mp, H)] if self.lo > 0 else None
        self.e = f(Mp, QPAD)
        self.nv, self.alpha, self.den = f(Nx, H), f(N, Lr), f(N)
        Rt = N + B
        self.Rt = Rt
        if self.dyprem is not None:
            self.dyprem, self.dh1prem = z(Mp, H), z(Mp, H)
        self.S = f(Rt, D)                 # student rows: [B*U history | B*C candidate | B user]
        self.dS = f(Rt, D)
        self.Sv, self.dSv = f(N, D), f(N, D)      # vectors / gradients per DISTINCT news of the step (dedup.py)
        self.plan = None
        T_ = max(cfg.T, 1)
        self.X = f(T_, Rt, D)             # teacher rows, same layout
        self.Pm = f(T_, Rt, D)
        self.dP = f(T_, Rt, D)
        self.ones = torch.ones(Rt, device=dev)
        self.hidx = torch.arange(B * cfg.U, device=dev, dtype=torch.int32).view(B, cfg.U)
        self.cidx = (B * cfg.U + torch.arange(B * cfg.C, device=dev, dtype=torch.int32)).view(B, cfg.C)
        self.score, self.dscore = f(B, cfg.C), f(B, cfg.C)
        self.e_u, self.alpha_u, self.den_u = f(B, cfg.U, cfg.Qu), f(B, cfg.U), f(B)
        self.t_score = f(T_, B, cfg.C)
        self.e_t, self.alpha_t, self.den_t = f(T_, B, cfg.U, cfg.Qu), f(T_, B, cfg.U), f(T_, B)
        self.tw = f(B, T_)
        self.losses = f(4)
        self.kd_part = f(Rt)
        self.user_part = f(B, T.query("tnr_user_bwd_part_stride", D, cfg.Qu))     # [b1 | w2 | pad | b2] per impression
        self.hv_u, self.dhv_u, self.dpre_u = f(B * cfg.U, D), f(B * cfg.U, D), f(B * cfg.U, cfg.Qu)
        if cfg.nrms_heads:
            BU, BC = B * cfg.U, B * cfg.C
            mk = lambda nm: (f(nm, BU, D), f(nm, BU, 3 * D), f(nm, BU + BC, D))          # blended rows, q|k|v, [ctx | candidates]
            self.nr_s, self.nr_t = mk(1), mk(T_)
            self.nr_dctx, self.nr_dqkv, self.nr_dhv = f(BU, D), f(BU, 3 * D), f(BU, D)
            self.ones_mask = torch.ones((B, cfg.U), device=dev)
            self.hpos = torch.arange(BU, device=dev, dtype=torch.int32).view(B, cfg.U)
            self.cpos = (BU + torch.arange(max(BC, 1), device=dev, dtype=torch.int32))[:BC].view(B, cfg.C)
        # backward buffers
        self.dnv = f(Nx, H)
        self.dy, self.dy2 = z(Mp, H), z(Mp, H)
        self.dpre = z(Mp, QPAD)
        self.dw2p, self.db2p = f(Nx, cfg.Qn), f(Nx)
        self.dypre, self.dh1, self.dh1pre, self.dctx = z(Mp, H), z(Mp, H), z(Mp, H), z(Mp, H)
        self.du = z(Mp, I)
        self.dqkv = z(Mp, 3 * H)
        # partial sums of the bias / LayerNorm gradients: a set per trainable layer, so that ONE batched reduction at the end of the
        # backward can sum them all (they are a few tens of MB per layer)
        self.lpart = {l: dict(ln_part=f(T.query("tnr_ln_bwd_part_elems", Mp, H)), ln_part1=f(T.query("tnr_ln_bwd_part_elems", Mp, H)),
                              gcs_part=f(T.query("tnr_gemm_colsum_rows", Mp), I), qkvb_part=f(Nx, 3 * H), cs_tmp=f(I))
                      for l in cfg.trainable_layers}
        if cfg.train_embeddings:
            # embedding backward: fp32 gradient rows of the summed embeddings (N L H 4 bytes), its [dgamma | dbeta] partials, the
            # column-sum partials of the position rows ((N, L H) view) and of the token-type row
            self.dx_emb = f(Mp, H)
            self.emb_part = f(T.query("tnr_embed_ln_bwd_part_elems", Mp, H))
            self.emb_cs_part = f(max(T.query("tnr_colsum_part_elems", max(Nx, 1), L * H), T.query("tnr_colsum_part_elems", L, H),
                                     T.query("tnr_colsum_part_elems", Mp, H)))
        self.red = {}                                                      # gradient bucket -> _ReduceBatch
        self.cs_part = f(max(T.query("tnr_colsum_part_elems", Mp, 3 * H if L > 32 else QPAD),
                             T.query("tnr_colsum_part_elems", 128, I),
                             T.query("tnr_colsum_part_elems", max(B * cfg.U, 1), 3 * D),
                             T_ * T.query("tnr_colsum_part_elems", Rt, D)))
        self.db1p = f(Nx, QPAD)
        # chunked pooling kernels for few, long sequences (stage-1 bodies): their workspace
        self.ap_ws = f(T.query("tnr_attpool_long_ws_elems", N, L, H, cfg.Qn, QPAD)) if (L > AP_LONG and cfg.pooling == "att") else None
        self.epre_u = f(B * cfg.U, cfg.Qu)
        self.epad_buf = {1: f(1, cfg.Qu), T_: f(T_, cfg.Qu)}      # student / teachers (these run on different streams)
        self.epre_t = f(T_, B * cfg.U, cfg.Qu)
        self.KS = 8                                                        # split-K of the long-K small GEMMs
        # x 2: the K-split members of a grouped launch get disjoint slices (_sgemm_group)
        self.sg_part = f(2 * self.KS * max(T_ * D * D, D * H, 3 * D * D, T_ * Rt * D, N * max(H, D), T_ * B * cfg.U * max(cfg.Qu, 3 * D)))
        self.sg_part2 = f(self.KS * max(cfg.Qu * D, 3 * D * D if cfg.nrms_heads else 1))       # second split problem of a grouped launch
        # weight-gradient slabs: the four gradients of a layer are in flight together (_wgrad_flush), each with slabs of its own
        self.ws = f(max(sum(_rup(self._wgrad_splits(n_, k_)[1], 64) for n_, k_ in ((3 * H, H), (H, H), (I, H), (H, I))),
                        self._wgrad_splits(QPAD, H)[1]))
        self._rel_stale = True       # filled by the first encode() (no kernel launch at construction time)

    WGRAD_UNITS = 1     # work units (split, tile) per workgroup of the queue-fed weight-gradient kernel.  1 = one full round
                        # (fastest alone).  Beside CUs held by an overlapped all-reduce a late workgroup costs a whole unit:
                        # x1.65 at 1, x1.25 at 2, x1.1-1.15 at 4 -- but every doubling adds a round of fp32 slab traffic
                        # (alone: +10 % at 2, +24 % at 4 for the 3072 x 768 gradient; tools/cu_contention.py)

    merge_reductions = True   # False: the partial-sum reductions per gradient bucket even without a bucket hook (tools/step_ab.py)
    group_wgrad = False  # True: a layer's weight gradients in one persistent launch (tnr_gemm_tn_wgrad_group; the same bits).  Measured
                         # on one GPU: step +6.4 %, the four gradients 848 -> 1 088 us (EXPERIMENTS.md section 4 item 22) - one launch each,
                         # one unit per workgroup, all units equal and in lockstep, is the better schedule; kept as a switch for the
                         # data-parallel case, where a workgroup held off its CU by a collective costs a quarter of what it costs now
    _wg = None           # the collected weight gradients while a layer's backward runs
    _wg_defer = None     # ... while a backward runs step by step beside another engine's (backward_encoder_steps)
    sg_kdiv = 256        # K per split of the small fp32 GEMMs (_sgemm_problem; 128 was 0.3 % slower: `AB=sg_kdiv:128:256 tools/step_ab.py`)
    group_sgemm = True   # False: the independent fp32 GEMMs of the heads one tnr_sgemm each (_sgemm_group; `AB=group_sgemm:0:1 tools/step_ab.py`)
    fused_user_fwd = True    # False: fc1 of the user encoders as fp32 GEMMs in front of tnr_user_score_fwd, four launches more per pass (EXPERIMENTS.md, tools/scratch/uf_time.py)
    _ib_on = False           # the last forward ran with in-batch negatives (forward(inbatch_ids=...)): backward adds their gradient
    _inbatch = None          # ... and their buffers, made on first use (_inbatch_buffers)
    teacher_stream = None    # a torch.cuda.Stream: the teacher side of the forward on it; no gain measured (`AB=teacher_stream:0:1 tools/step_ab.py`)
    fcache = None        # build_frozen_cache(): (hidden states entering layer lo, additive masks, the table's _table_key, its rows, the table)
    _pos_cache = None    # _pos_ids(): (_table_key, position ids, the table) of the resident token table
    _red_ginv = None     # _red_check(): the 1 / (loss scale) the recorded reduction tables carry
    dyprem = dh1prem = None  # set_dropout(): the masked LayerNorm-backward outputs, allocated by the first call that turns dropout on
    nr_s = nr_t = None   # _alloc_workspace() under nrms_heads: the student's / teachers' (blended rows, q|k|v, [ctx | candidates])

    @staticmethod
    def _wgrad_splits(N, K, units=None):
        """-> (splits over M, workspace elems): `units` (default Engine.WGRAD_UNITS) rounds of workgroups on the 256 CUs (one
        256x256 output tile x split each); more splits only add fp32 slab traffic (N*K*4 B written and re-read per split)."""
        tiles = (N // 256) * (K // 256) if (N % 256 == 0 and K % 256 == 0) else (N // 128) * (K // 128)
        splits = max(1, min(64, (units or Engine.WGRAD_UNITS) * 256 // max(tiles, 1)))
        return splits, T.query("tnr_gemm_tn_ws_elems", N, K, splits)

    # ------------------------------------------------------------------ kernel wrappers
    def _gemm(self, a, w, c, M, bias=None, res=None, aux=None, flags=0, colsum=None, drop=None, drop_tail=None, split_row=None):
        """drop_tail / split_row: rows [split_row, M) under the site drop_tail (tnr_gemm_nt_do_split; a second part's rows)."""
        N, K = w.shape
        args = (a, a.stride(0), w, w.stride(0), c, c.stride(0), M, N, K, bias, res,
                res.stride(0) if res is not None else 0, aux, aux.stride(0) if aux is not None else 0, flags, colsum)
        if drop is None:
            self._c("tnr_gemm_nt_ex", *args)
        elif drop_tail is not None:
            self._c("tnr_gemm_nt_do_split", *args, drop, drop_tail, split_row)
        else:
            self._c("tnr_gemm_nt_do", *args, drop)

    def _wgrad(self, dy, x, dw, M, acc=0):
        N, K = dw.shape
        if self._wg is not None:           # inside a layer's backward: collected, launched together by _wgrad_flush
            self._wg.append((dy, x, dw, M, N, K, acc))
            return
        if self._wg_defer is not None:     # stage 1: collected for a launch shared with the other pass's (Stage1Engine.backward)
            self._wg_defer.append((dy, x, dw, M, N, K, acc))
            return
        self._c("tnr_gemm_tn_wgrad_ex", dy, dy.stride(0), x, x.stride(0), dw, dw.stride(0), M, N, K, self.ws,
               self._wgrad_splits(N, K)[0], acc, self.ginv)

    def _wgrad_flush(self, shared_round=False):
        """The weight gradients collected since the last flush in ONE persistent launch (+ one slab-sum launch): their (split, tile)
        units share a queue, so the workgroups that finish one gradient's units go on with the next one's instead of idling to the
        launch boundary, and a workgroup kept off its CU by another stream's kernel costs a unit of up to four rounds' worth
        instead of a whole round.  Each gradient is computed exactly as by its own launch (slabs of its own in self.ws).
        shared_round (stage 1's joint passes: few rows, 8 896 at 30 / 128): a full round of units per gradient (_wgrad_splits) would
        mean 20 m steps per unit, 7 fp32 slabs and a slab sum per gradient - instead ALL the collected gradients (at most four, of
        256 x 256 tiles) share ONE round: the same number of splits each, so every unit runs the same number of m steps."""
        pend, self._wg = self._wg, []
        if not pend:
            return
        if shared_round:
            assert len(pend) <= 4 and all(N % 256 == 0 and K % 256 == 0 for _, _, _, _, N, K, _ in pend)
            shared = max(1, min(64, (256 * Engine.WGRAD_UNITS) // sum((N // 256) * (K // 256) for _, _, _, _, N, K, _ in pend)))
        probs, off = [], 0
        for dy, x, dw, M, N, K, acc in pend:
            splits, elems = (shared, T.query("tnr_gemm_tn_ws_elems", N, K, shared)) if shared_round else self._wgrad_splits(N, K)
            probs.append(dict(dY=dy, lddy=dy.stride(0), X=x, ldx=x.stride(0), dW=dw, lddw=dw.stride(0), M=M, N=N, K=K,
                              ws=self.ws[off:off + elems], splits=splits, accumulate=acc, out_scale=self.ginv))
            off += _rup(elems, 64)
        assert off <= self.ws.numel()
        for i in range(0, len(probs), 4):
            T.wgrad_group(probs[i:i + 4], f16=self.f16)

    def _colsum(self, x, out, M, dtype=T.BF16):   # dtype BF16 = "the 16-bit type of the build"
        self._c("tnr_colsum", x, x.stride(0), dtype, M, x.shape[1], out, self.cs_part, 0)

    def _sgemm(self, A, a_rs, a_cs, sA, Bm, b_rs, b_cs, sB, C, ldc, sC, bias, sBias, M, N, K, batch=1, ksplit=None, alpha=1.0,
               beta=0.0):
        """One fp32 GEMM in a launch of its own (tnr_sgemm); a K split takes its partial sums through self.sg_part."""
        self._sgemm_call(self._sgemm_problem(A, a_rs, a_cs, sA, Bm, b_rs, b_cs, sB, C, ldc, sC, bias, sBias, M, N, K, batch, ksplit,
                                             alpha, beta, part=self.sg_part))

    def _sgemm_problem(self, A, a_rs, a_cs, sA, Bm, b_rs, b_cs, sB, C, ldc, sC, bias, sBias, M, N, K, batch=1, ksplit=None, alpha=1.0,
                       beta=0.0, part=None):
        """The arguments of _sgemm as one member of a grouped launch (T.sgemm_group: independent small GEMMs in one launch, each
        computed exactly as its own tnr_sgemm call would).  A split problem needs a partial buffer of its own (`part`).
        ksplit None: K is split into slices of >= sg_kdiv = 256 (a workgroup's time on the fp32 MFMA is ~K * 32 cycles whatever the
        tile count, and these GEMMs have few tiles; slices of 128 cost a split-reduce launch for the K = 256 GEMMs and were 0.3 %
        slower on the step, `AB=sg_kdiv:128:256 tools/step_ab.py`).  The split depends on K ALONE, never on the row count: a news vector must
        come out with the same bits whatever batch it is encoded in (in-batch de-duplication, frozen-layer cache)."""
        if ksplit is None:
            ksplit = max(1, min(K // self.sg_kdiv, 8))
        if ksplit > 1 and part is not None:
            assert ksplit * batch * M * N <= part.numel(), "fp32 GEMM workspace too small for its K split"
        return dict(A=A, a_rs=a_rs, a_cs=a_cs, sA=sA, B=Bm, b_rs=b_rs, b_cs=b_cs, sB=sB, C=C, ldc=ldc, sC=sC, bias=bias, sBias=sBias,
                    M=M, N=N, K=K, batch=batch, alpha=alpha, beta=beta, ksplit=ksplit, part=part if ksplit > 1 else None)

    def _sgemm_call(self, q):
        """A problem of _sgemm_problem as its own tnr_sgemm launch: the one place that spells the entry point's argument order."""
        T.call("tnr_sgemm", q["A"], q["a_rs"], q["a_cs"], q["sA"], None, q["B"], q["b_rs"], q["b_cs"], q["sB"], q["C"], q["ldc"], q["sC"],
               q["bias"], q["sBias"], q["M"], q["N"], q["K"], q["batch"], q["alpha"], q["beta"], q["ksplit"], q["part"])

    def _sgemm_group(self, problems):
        """Independent fp32 GEMMs in one launch (Engine.group_sgemm = False: one tnr_sgemm each, the same bits; tools/step_ab.py).
        The members run concurrently, so every K-split member gets a DISJOINT slice of the partial buffer (tnr_sgemm_group:
        'not shared inside a group'); a member that brought its own buffer keeps it."""
        off = 0
        for q in problems:
            if q["ksplit"] > 1 and q["part"] is None:
                need = q["ksplit"] * q["batch"] * q["M"] * q["N"]
                q["part"] = self.sg_part[off:off + need]
                off += _rup(need, 64)
        assert off <= self.sg_part.numel(), "fp32 GEMM workspace too small for the K splits of a grouped launch"
        parts = [q["part"].data_ptr() for q in problems if q["part"] is not None]
        assert len(parts) == len(set(parts)), "two members of a grouped fp32 GEMM share a partial buffer"
        if self.group_sgemm:
            T.sgemm_group(problems)
            return
        for q in problems:
            self._sgemm_call(q)

    # ------------------------------------------------------------------ forward
    def build_frozen_cache(self, news_combined):
        """The layers below the first trainable one never change during training (run.py:101-112), so for a resident
        news table their output is a function of the news id alone: compute it ONCE for every row -- hidden states
        entering layer `lo` (n+1, L*H) 16-bit, 2.4 GB for 51 k titles, plus the additive masks -- and let encode() gather
        rows instead of re-running the embedding and the frozen layers every step.  Bit-identical to recomputing
        (rows are processed independently); the reference recomputes, bench.py's headline does too.
        The entry is for THIS table as it is now: it keeps the table tensor (its address cannot be handed out again while the
        entry lives) and its _table_key - address, shape, dtype and torch's version counter - and encode() takes the cache only
        for a table with that key.  A table rewritten in place through torch (copy_), another table, a view with fewer rows:
        a miss, which recomputes like any foreign table; call this again to cache the new contents."""
        self.fcache = None
        if self.lo == 0:
            return False
        n, L, H = news_combined.shape[0], self.cfg.L, self.cfg.H
        fx = torch.empty((n, L * H), device=self.dev, dtype=self.tdt)
        fm = torch.empty((n, self.Lr), device=self.dev, dtype=torch.float32)
        cap = self.N_alloc
        for s0 in range(0, n, cap):
            cnt = min(cap, n - s0)
            idx = torch.arange(s0, s0 + cnt, device=self.dev, dtype=torch.int32)
            x = self.encode(news_combined, cnt, nidx=idx, stop_at=self.lo, train=False)
            fx[s0:s0 + cnt].copy_(x[:cnt * L].view(cnt, L * H))
            fm[s0:s0 + cnt].copy_(self.mask_add[:cnt])
        self.fcache = (fx.view(torch.float32), fm, self._table_key(news_combined), n, news_combined)
        return True

    @staticmethod
    def _table_key(tok):
        """What an entry cached for a resident table is valid for: (address, shape, dtype, version counter).  torch counts every
        in-place write it makes to the storage (a view shares its base's counter), so a table refreshed by copy_ is another key;
        whoever caches under it keeps `tok` itself beside the entry, so that no other table can get the address.  A kernel that
        writes the table through its raw pointer is not counted - rebuild the caches after one."""
        return (tok.data_ptr(), tuple(tok.shape), tok.dtype, tok._version)

    def _pos_ids(self, tok):
        """RoBERTa position ids of a token table (rows [ids | mask], any integer dtype) -> (rows, L) int32; the resident table's
        are computed once and served again for a table with the same _table_key (a view of the whole unchanged table hits; one
        with fewer rows, the table rewritten in place, or another table at an address that was free again does not: the entry
        keeps the table tensor).  Integer index preparation, like the torch.cat of the news indices."""
        key = self._table_key(tok)
        c = self._pos_cache
        if c is not None and c[0] == key:
            return c[1]
        L, pad = self.cfg.L, self.cfg.pos_pad_id
        ne = (tok[:, :L] != pad)
        pid = (torch.cumsum(ne.to(torch.int32), 1) * ne + pad).to(torch.int32).contiguous()
        if tok.shape[0] > 4 * self.N_alloc:          # a resident table, not a per-step batch
            self._pos_cache = (key, pid, tok)
        return pid

    # encode() and backward_encoder_steps() work on a list of PARTS laid one behind the other in this engine's per-token buffers:
    # (engine, sequences, first token row, first sequence row).  One pass is one part, [(self, n_seq, 0, 0)]; stage 1's joint passes
    # are two, the body engine's behind the title engine's, with the title engine as host (stage1.py).  Every Linear, LayerNorm and
    # weight gradient is one launch over all parts' rows; what depends on the sequence length - the pieces below, with their
    # per-token operands explicit - runs once per part on that part's rows, through the part's engine (its L, masks, statistics).
    def _per_part(self, parts, side, fn):
        """fn(engine, sequences, first row, first sequence) per part.  Two parts: the one behind first (stage 1 encodes the bodies
        first), on the stream `side` beside the other if there is one."""
        if len(parts) == 1:
            fn(*parts[0])
        else:
            _fork_join(side, lambda: fn(*parts[1]), lambda: fn(*parts[0]))

    def _parts_state(self, parts, N, side, **more):
        """What the launches of one encode() / backward over `parts` share, built once per call (a plain record, no behaviour)."""
        two = len(parts) > 1
        return SimpleNamespace(
            parts=parts, side=side, two=two, N=N,
            M0=N * self.cfg.L,                                # rows of the first part: where a second one's begin
            M=sum(n * e.cfg.L for e, n, _, _ in parts), Ns=sum(n for _, n, _, _ in parts),
            ds=self._dsite,                                   # dropout sites of this part's current forward call (self.drop_cur)
            ds2=parts[1][0]._dsite if two else None,          # ... and of the second part's, for the rows from M0 on (_gemm, _ln_bwd)
            **more)

    def _embed_fwd(self, tok, n_seq, nidx, x0):
        cfg, g, ds = self.cfg, self.p, self._dsite
        L, H = cfg.L, cfg.H
        emb = (g(BERT + "embeddings.word_embeddings.weight"), g(BERT + "embeddings.position_embeddings.weight"),
               g(BERT + "embeddings.token_type_embeddings.weight"), g(BERT + "embeddings.LayerNorm.weight"),
               g(BERT + "embeddings.LayerNorm.bias"), cfg.ln_eps, x0, self.mask_add)
        de = ds(T.DROP_EMB, 0)
        pid = self._pos_ids(tok if nidx is not None else tok[:n_seq]) if cfg.pos_pad_id is not None else None
        name, args = ("tnr_embed_ln_fwd", (tok, n_seq, L, H, *emb)) if nidx is None else \
            ("tnr_embed_ln_fwd_indexed", (tok, nidx, n_seq, L, H, *emb))
        self._c(name + "_do", *args, de, pid) if (de or pid is not None) else self._c(name, *args)

    def _attn_fwd(self, qkv, ctx, lse, n_seq, dp):
        cfg = self.cfg
        name, args = ("tnr_attn_l32_fwd", (qkv, self.mask_add, self.rel, ctx, n_seq, cfg.L, cfg.A)) if cfg.L <= 32 else \
            ("tnr_attn_long_fwd", (qkv, self.mask_add, self.rel, ctx, lse, n_seq, cfg.L, cfg.A))
        self._c(name + "_do", *args, dp) if dp else self._c(name, *args)

    def _attpool_fwd(self, x, e, nv, n_seq):
        cfg, g = self.cfg, self.p
        args = (x, e, QPAD, g(PFX + "attn.att_fc2.weight"), g(PFX + "attn.att_fc2.bias"), cfg.Qn, nv, self.alpha, self.den)
        if cfg.L > AP_LONG:                  # few, long sequences (stage-1 bodies): the chunked kernels fill the chip
            self._c("tnr_attpool_fwd_long", *args, self.ap_ws, n_seq, cfg.L, cfg.H)
        else:
            self._c("tnr_attpool_fwd", *args, n_seq, cfg.L, cfg.H)

    def _attpool_bwd(self, y, e, dnv, dy2, dpre, dw2p, db2p, db1p, n_seq):
        cfg, g = self.cfg, self.p
        args = (y, e, QPAD, g(PFX + "attn.att_fc2.weight"), cfg.Qn, dnv, self.alpha)
        outs = (dy2, dpre, QPAD, dw2p, db2p, db1p)
        if cfg.L > AP_LONG:
            self._c("tnr_attpool_bwd_long", *args, *outs, self.ap_ws, n_seq, cfg.L, cfg.H)
        else:
            self._c("tnr_attpool_bwd", *args, self.den, *outs, n_seq, cfg.L, cfg.H)

    def _attn_bwd(self, qkv, ctx, lse, dctx, dqkv, qkvb_part, n_seq, dPb):
        """-> True if the q/k/v bias partial sums came out of the kernel (L <= 32), False if the caller sums dqkv's columns."""
        cfg = self.cfg
        short = cfg.L <= 32
        name, args = ("tnr_attn_l32_bwd", (qkv, self.mask_add, self.rel, dctx, dqkv, qkvb_part, n_seq, cfg.L, cfg.A)) if short else \
            ("tnr_attn_long_bwd", (qkv, self.mask_add, self.rel, ctx, dctx, lse, self.delta, dqkv, n_seq, cfg.L, cfg.A))
        self._c(name + "_do", *args, dPb) if dPb else self._c(name, *args)
        return short

    def encode(self, tok, n_seq, nidx=None, out=None, stop_at=None, train=True, extra=None, parts=None, src2=None, side=None,
               before=None):
        """NewsEncoder.forward model_bert.py:119-137 -> news vectors S[:n_seq] (fp32).
        tok (n_seq, 2L) int64 on device, or (nidx given) tok = resident news_combined (n+1, 2L) int32 and
        nidx (n_seq,) int32 news indices.  stop_at = l: return the hidden states entering layer l instead.
        parts (two, this engine's first: see _per_part): the second part's sequences, src2 = its (tok, nidx), go through the same
        launches behind this one's, their news vectors to S[n_seq:]; side = the stream of its own kernels or None; before() is
        called directly in front of this part's embedding launch (work of the caller's that runs beside the part behind)."""
        cfg = self.cfg
        s = self._parts_state(parts or [(self, n_seq, 0, 0)], n_seq, side)
        assert s.M <= self.Mp and s.Ns <= self.nv.shape[0]
        for e, _, _, _ in s.parts:
            if e._rel_stale:
                e.refresh_rel()
            e._begin_drop_call(train)                         # each part its own numbered forward call
        fc = self.fcache if self.drop_cur is None else None   # a cached prefix has no fresh masks
        assert not s.two or (fc is None and stop_at is None and out is None and not extra and cfg.pooling == "att")
        first = 0
        if fc is not None and nidx is not None and stop_at is None and self._table_key(tok) == fc[2]:
            # frozen prefix from the per-news cache (build_frozen_cache): two row gathers replace embedding + lo layers
            T.call("tnr_gather_rows", fc[0], fc[3], nidx, n_seq, fc[0].shape[1], 1, self.x0.view(torch.float32), n_seq, 0)
            T.call("tnr_gather_rows", fc[1], fc[3], nidx, n_seq, self.Lr, 1, self.mask_add, n_seq, 0)
            first = self.lo
        else:
            self._emb_src = (tok, nidx, n_seq)                # what _embed_bwd addresses the tokens by
            def embed(e, n, r0, s0):
                if r0:
                    e._embed_fwd(src2[0], n, src2[1], self.x0[r0:])
                    return
                if before:
                    before()
                e._embed_fwd(tok, n, nidx, self.x0)
            self._per_part(s.parts, side, embed)
        x = self.x0
        self.x_in = {}
        for l in range(first, cfg.n_layers):
            if stop_at is not None and l == stop_at:
                return x
            x = self._layer_fwd(s, l, x)
        self.y_last = x
        return self._head_fwd(s, x, out, extra)

    def _layer_fwd(self, s, l, x):
        """Encoder layer l (tnlrv3/modeling.py BertLayer): x -> y.  A layer from lo on keeps its activations for the backward (and its
        input in x_in); a frozen one below works in the scratch set and alternates between the two scratch outputs."""
        cfg, g, ds, ds2 = self.cfg, self.p, s.ds, s.ds2
        H, M = cfg.H, s.M
        names, sh = self.lnames[l], self.sh[l]
        kept = l >= self.lo
        a = self.act[l - self.lo] if kept else self.scr
        y = a["y"] if kept else self.scr_y[l & 1]
        self.x_in[l] = x
        self._gemm(x, sh["qkv"], a["qkv"], M, bias=self._view(names[3], 3 * H, (3 * H,)), flags=T.EPI_BIAS)

        def attn(e, n, r0, s0):
            e._attn_fwd(_from(a["qkv"], r0), _from(a["ctx"], r0), e.act[l - e.lo]["lse"] if kept else e.lse, n,
                        e._dsite(T.DROP_PROB, l))
        self._per_part(s.parts, s.side, attn)
        self._gemm(a["ctx"], sh["o"], a["h1pre"], M, bias=g(names[7]), res=x, flags=T.EPI_BIAS | T.EPI_RES,
                   drop=ds(T.DROP_ATTN_OUT, l), drop_tail=ds2(T.DROP_ATTN_OUT, l) if s.two else None, split_row=s.M0)
        self._c("tnr_ln_fwd", a["h1pre"], g(names[8]), g(names[9]), cfg.ln_eps, a["h1"], a["st1"], M, H)
        fl = T.EPI_BIAS | T.EPI_GELU | (T.EPI_AUXOUT if kept else 0)
        self._gemm(a["h1"], sh["w1"], a["g"], M, bias=g(names[11]), aux=a["u"] if kept else None, flags=fl)
        self._gemm(a["g"], sh["w2"], a["ypre"], M, bias=g(names[13]), res=a["h1"], flags=T.EPI_BIAS | T.EPI_RES,
                   drop=ds(T.DROP_FFN_OUT, l), drop_tail=ds2(T.DROP_FFN_OUT, l) if s.two else None, split_row=s.M0)
        self._c("tnr_ln_fwd", a["ypre"], g(names[14]), g(names[15]), cfg.ln_eps, y, a["st2"], M, H)
        return y

    def _head_fwd(self, s, x, out, extra):
        """Pooling (model_bert.py:130-135: AttentionPooling without mask | token 0 | mean) + dense (:136) of the news encoder:
        the last layer's output x -> news vectors in `out` (None: self.S)."""
        cfg, g = self.cfg, self.p
        H = cfg.H
        if cfg.pooling == "att":
            self._gemm(x, self.sh_a1, self.e, s.M, bias=self.b_a1, flags=T.EPI_BIAS | T.EPI_TANH | T.EPI_OUTF32)
            self._per_part(s.parts, s.side, lambda e, n, r0, s0: e._attpool_fwd(_from(x, r0), _from(self.e, r0), _from(self.nv, s0), n))
        else:
            self._c("tnr_pool_fwd", x, self.nv, s.N, cfg.L, H, int(cfg.pooling == "mean"))
        dst = self.S if out is None else out
        dense = (self.nv, H, 1, 0, g(PFX + "dense.weight"), H, 1, 0, dst, cfg.D, 0, g(PFX + "dense.bias"), 0, s.Ns, cfg.D, H)
        if extra:      # independent fp32 GEMMs the caller had pending (the teachers' projection): one launch with the dense layer
            self._sgemm_group([self._sgemm_problem(*dense)] + list(extra))
        else:
            self._sgemm(*dense)
        return dst[:s.Ns]

    # ------------------------------------------------------------------ forward-only paths
    @torch.no_grad()
    def encode_news(self, news_combined):
        """news_scoring of run.py:276-287 / :438-444: every row of the resident token table (n+1, 2L) int32
        through NewsEncoder.forward, in passes of the workspace's sequence capacity.  -> (n+1, D) fp32."""
        n = news_combined.shape[0]
        cap = self.N_alloc
        out = torch.empty((n, self.cfg.D), device=self.dev, dtype=torch.float32)
        for s0 in range(0, n, cap):
            cnt = min(cap, n - s0)
            idx = torch.arange(s0, s0 + cnt, device=self.dev, dtype=torch.int32)
            out[s0:s0 + cnt].copy_(self.encode(news_combined, cnt, nidx=idx, train=False))
        return out

    @torch.no_grad()
    def user_vectors(self, news_scoring, hist_idx, history_mask):
        """student.user_encoder(log_vecs, log_mask) of run.py:343 on rows of news_scoring gathered by index.
        hist_idx (B,U) int32, mask (B,U) -> (B,D) fp32 (B <= the engine's batch)."""
        cfg = self.cfg
        B, U, D, Qu = hist_idx.shape[0], cfg.U, cfg.D, cfg.Qu
        assert B <= self.B_alloc and hist_idx.shape[1] == U
        g, ue = self.p, "student.user_encoder."
        rows = self.X[0, :B * U]                                   # scratch: gathered history rows
        T.call("tnr_gather_rows", news_scoring, news_scoring.shape[0], hist_idx.reshape(-1).contiguous(), B * U, D, 1, rows,
               B * U, 0)
        hidx = self.hidx[:B]
        mask = history_mask.to(torch.float32).contiguous()
        self._user_forward(rows, B * U, 1, self._user_params(ue, 1), hidx, hidx, mask, self.epre_u, self.dS, B * D, self.score,
                           self.e_u, self.alpha_u, self.den_u, B, 0, self.nr_s)
        return self.dS[:B].clone()

    @torch.no_grad()
    def topk(self, users, news_scoring, k, exclude=None, first_row=1, splits=0):
        """Of all rows of news_scoring (Nn, D), the k each user should see (tnr_topk_scores, include/tnr_hip.h): scores on the
        exact fp32 MFMA, selection fused behind them, the (Nu, Nn) score matrix never exists.  users: any fp32 (Nu, D) device
        tensor; exclude: int32 (Nu, E) rows never to return (ids < first_row, e.g. the padding 0, are ignored).
        -> (idx int32 (Nu, k), score fp32 (Nu, k)), best first, ties to the lower row, idx -1 / score -inf where fewer than k
        rows are eligible.  The workspace is a torch allocation of the size the library states, cached by size."""
        assert users.dtype == torch.float32 and news_scoring.dtype == torch.float32 and users.dim() == 2 and news_scoring.dim() == 2
        assert users.shape[1] == news_scoring.shape[1] and users.stride(1) == 1 and news_scoring.stride(1) == 1
        Nu, D = users.shape
        Nn = news_scoring.shape[0]
        e_rs = E = 0
        if exclude is not None:
            assert exclude.shape[0] == Nu and exclude.dim() == 2
            exclude = exclude.to(device=users.device, dtype=torch.int32)
            if exclude.stride(1) != 1:
                exclude = exclude.contiguous()
            e_rs, E = exclude.stride(0), exclude.shape[1]
        idx = torch.empty((Nu, k), device=users.device, dtype=torch.int32)
        score = torch.empty((Nu, k), device=users.device, dtype=torch.float32)
        nbytes = int(T.query("tnr_topk_workspace", Nu, Nn, k, splits))
        cache = self._topk_ws
        work = cache.get(nbytes)
        if work is None:
            cache.clear()                                          # one size at a time: serving batches repeat their shape
            work = cache[nbytes] = torch.empty((max(nbytes, 8),), device=users.device, dtype=torch.uint8)
        T.call("tnr_topk_scores", users, users.stride(0), Nu, news_scoring, news_scoring.stride(0), Nn, first_row, D,
               exclude if E else None, e_rs, E, k, idx, score, splits, work, nbytes)
        return idx, score

    @torch.no_grad()
    def recommend(self, news_scoring, hist_idx, history_mask, k, exclude_history=True):
        """user_vectors(...) followed by topk over the whole table (row 0, the padding news, is never returned): the serving
        step.  exclude_history: the user's clicked rows are not recommended again (hist_idx's padding zeros match nothing).
        B <= the engine's batch; every buffer and counter is left as user_vectors leaves it."""
        users = self.user_vectors(news_scoring, hist_idx, history_mask)
        return self.topk(users, news_scoring, k, exclude=hist_idx if exclude_history else None, first_row=1)

    @torch.no_grad()
    def rank_metrics(self, users, news_scoring, cands, labels, acc=None, per=False, offs=None):
        """AUC, MRR, nDCG@5 and nDCG@10 of a batch of impressions on the device (tnr_rank_metrics, include/tnr_hip.h): row b of
        users (B, D) against the rows of news_scoring (Nn, D) that impression b lists, with run.test's skip rule (no positive or
        no negative) and metrics.py's tie rule.  cands / labels: the eval loader's lists of numpy arrays, packed by
        pack_impressions and uploaded in one copy - or int32 device tensors already packed, with offs (B + 1) beside them.
        acc: a float64 (6,) device tensor {seen, scored, sum AUC, sum MRR, sum nDCG@5, sum nDCG@10} to add this batch's totals
        to; None starts a new one.  -> (acc, scores fp32 (all candidates), per (B, 4) float64 or None).  Nothing is read back."""
        assert users.dtype == torch.float32 and news_scoring.dtype == torch.float32 and users.dim() == 2 and news_scoring.dim() == 2
        assert users.shape[1] == news_scoring.shape[1] and users.stride(1) == 1 and news_scoring.stride(1) == 1
        B, D = users.shape
        Nn = news_scoring.shape[0]
        dev = users.device
        if isinstance(cands, torch.Tensor):
            assert offs is not None and offs.numel() == B + 1, "packed impressions come with their offsets"
            cand, label, offs = (x.to(device=dev, dtype=torch.int32).contiguous() for x in (cands, labels, offs))
            assert cand.numel() == label.numel()
        else:
            assert len(cands) == B and len(labels) == B
            c, y, o = pack_impressions(cands, labels)
            if c.size and int(c.max()) >= Nn:
                raise ValueError("rank_metrics: candidate row %d outside the %d rows of news_scoring" % (int(c.max()), Nn))
            buf = torch.from_numpy(np.concatenate([o, c, y])).to(dev)          # the batch's one upload
            offs, cand, label = buf[:B + 1], buf[B + 1:B + 1 + c.size], buf[B + 1 + c.size:]
        n_cand = cand.numel()
        if n_cand == 0:                                                        # impressions without candidates: nothing is indexed,
            cand = label = torch.zeros((1,), device=dev, dtype=torch.int32)    # but the library refuses a null pointer
        scores = torch.empty((max(n_cand, 1),), device=dev, dtype=torch.float32)
        per_t = torch.empty((max(B, 1), 4), device=dev, dtype=torch.float64)   # always: the kernel's fast form keeps them there
        accumulate = acc is not None
        if acc is None:
            acc = torch.empty((6,), device=dev, dtype=torch.float64)
        assert acc.dtype == torch.float64 and acc.numel() == 6 and acc.is_contiguous() and acc.device == scores.device
        T.call("tnr_rank_metrics", users, users.stride(0), B, news_scoring, news_scoring.stride(0), Nn, D, offs, cand, label, scores,
               per_t, acc, 1 if accumulate else 0)
        return acc, scores[:n_cand], (per_t[:B] if per else None)

    @torch.no_grad()
    def evaluate(self, news_scoring, hist_idx, history_mask, cands, labels, acc=None, per=False):
        """user_vectors(...) followed by rank_metrics over each impression's candidates: one batch of run.test's loop without
        the host.  B <= the engine's batch; every buffer and counter is left as user_vectors leaves it."""
        users = self.user_vectors(news_scoring, hist_idx, history_mask)
        return self.rank_metrics(users, news_scoring, cands, labels, acc=acc, per=per)

    def _prepare(self, B):
        # buffers are sized for the exact batch: row strides of the stacked (T, Rt, D) arrays and the
        # zero rows the wgrad kernels rely on (rows [M, roundup(M,64))) both depend on it.  Only the last,
        # short batch of an epoch (streaming.py:76, no drop_remainder) ever changes B.
        if B != self.B_alloc:
            self._alloc_workspace(B)

    def _check_plan(self, plan, N):
        """A de-duplication plan (dedup.py) this step can run, for both feeds.  The 64-row rule: the weight-gradient kernels
        (tnr_gemm_tn_wgrad*) read dY and X up to roundup(M, 64) rows and need zeros behind row M.  An un-deduplicated pass has them:
        the workspace is laid out for its batch and nothing writes behind its rows.  A plan's M = n_enc * L rows lie INSIDE that
        workspace, with whatever an earlier, larger pass left directly behind them, so M itself has to be a multiple of 64 - which
        build_plan's default quantum of 64 sequences gives for every L, and another quantum in general does not."""
        L = self.cfg.L
        if plan.n_slots != N or not 0 < plan.n_enc <= N:
            raise ValueError("dedup plan for %d slots encoding %d sequences, but the batch has %d slots" % (plan.n_slots, plan.n_enc, N))
        if (plan.n_enc * L) % 64:
            raise ValueError("dedup plan encodes %d sequences x %d tokens = %d token rows, not a multiple of 64: the weight-gradient "
                             "kernels read up to the next multiple of 64 rows and would sum an earlier pass's rows into this step's "
                             "gradients; build the plan with quantum=64 (dedup.build_plan's default)" % (plan.n_enc, L, plan.n_enc * L))

    def forward_indexed(self, news_combined, hist_idx, history_mask, cand_idx, label, teacher_tables, plan=None, inbatch=False):
        """The same step fed the way the resident-table loader feeds it: news_combined (n+1, 2L) int32 and
        teacher_tables (T, n+1, D) fp32 stay in HBM; per step only hist_idx (B,U), cand_idx (B,C) int32 news
        indices, the mask and the labels arrive (dataloader.py:129-149 at index level).
        inbatch=True: in-batch negatives in the target loss (forward's inbatch_ids), with the indices themselves as the news ids."""
        return self.forward(None, history_mask, None, label, teacher_tables=teacher_tables, t_hidx=hist_idx,
                            t_cidx=cand_idx, news_combined=news_combined, plan=plan,
                            inbatch_ids=(hist_idx, cand_idx) if inbatch else None)

    def forward(self, history, history_mask, candidate, label, teacher_hist=None, teacher_cand=None,
                teacher_tables=None, t_hidx=None, t_cidx=None, news_combined=None, plan=None, inbatch_ids=None):
        """Model.forward model_bert.py:262-305.  Teacher embeddings either as the reference's lists of
        (B,U,D)/(B,C,D) tensors, or as resident tables (T,R,D) + int32 row ids (B,U)/(B,C).
        Returns the device tensor [distill, target, emb, -] and student_score (B,C).
        inbatch_ids = (hist_ids (B,U), cand_ids (B,C)) news ids: the target loss ranks each impression's positive against the other
        impressions' candidates as well (include/tnr_hip.h, tnr_inbatch_*: the five rules) - losses[1] is then
        the loss over that larger set, the distillation and embedding terms and student_score are what they are without it, and
        backward() adds the new term's gradient to the user and candidate rows.  None or False: the reference's loss, and not one
        call or buffer more."""
        cfg = self.cfg
        B = history_mask.shape[0]
        U, C, L, D, T_ = cfg.U, cfg.C, cfg.L, cfg.D, cfg.T
        if plan is not None:
            self._check_plan(plan, B * (U + C))      # before anything is launched or re-laid
        if inbatch_ids is None or inbatch_ids is False:
            inbatch_ids = None
        elif cfg.stage1:
            raise ValueError("inbatch_ids with stage1=True: stage 1 has no users and no target loss to extend")
        elif inbatch_ids is True or len(inbatch_ids) != 2 or tuple(inbatch_ids[0].shape) != (B, U) or tuple(inbatch_ids[1].shape) != (B, C):
            raise ValueError("inbatch_ids must be the pair (hist_ids (B, U), cand_ids (B, C)) of news ids: token rows carry none "
                             "(forward_indexed(inbatch=True) passes its indices)")
        self._prepare(B)
        N = B * (U + C)
        Rt = N + B
        self.cur = (B, N, Rt)
        self.mask = history_mask.to(torch.float32).contiguous()
        self.label = label.to(torch.int64).contiguous()
        self._ib_on = inbatch_ids is not None
        if self._ib_on:
            # ids only: nothing of the step is needed, so it leads the step
            ib = self._inbatch_buffers()
            ids = [x.to(device=self.dev, dtype=torch.int32).contiguous() for x in inbatch_ids]
            T.call("tnr_inbatch_plan", ids[0], ids[1], ib["elig"], ib["count"], ib["first_ws"], B, U, C)
        idx = None
        if news_combined is not None or teacher_tables is not None:
            if (t_hidx.dtype == torch.int32 and t_cidx.dtype == torch.int32 and t_hidx.is_contiguous() and t_cidx.is_contiguous()
                    and t_hidx.device == self.dev):
                idx = self.nidx_buf[:N]                  # no ATen kernel inside the step
                T.call("tnr_concat_i32", t_hidx, B * U, t_cidx, B * C, idx)
            else:
                idx = torch.cat([t_hidx.reshape(-1), t_cidx.reshape(-1)]).to(device=self.dev, dtype=torch.int32)
        self.nidx = idx
        # teacher side (frozen user encoders over the teachers' rows, projection by the transform matrices): independent of
        # the student's encoder pass; issued first (optionally on a second stream, TNR_TEACHER_STREAM=1)
        hidx, cidx = self._idx(B)
        main = torch.cuda.current_stream(self.dev) if self.dev.type == "cuda" else None
        if T_ > 0:
            side = self._side_stream()
            side.wait_stream(main)
            with torch.cuda.stream(side):
                if teacher_tables is not None:
                    T.call("tnr_gather_rows", teacher_tables, teacher_tables.shape[1], idx, N, D, T_, self.X, self.X.shape[1], 0)
                else:
                    for i in range(T_):
                        self.X[i, :B * U].copy_(teacher_hist[i].reshape(B * U, D))
                        self.X[i, B * U:N].copy_(teacher_cand[i].reshape(B * C, D))
                self._user_forward(self.X, self.X.shape[1], T_, self._user_params("teachers.0.", T_), hidx, cidx, self.mask,
                                   self.epre_t, self.X[0, N:], self.X.stride(0), self.t_score, self.e_t, self.alpha_t,
                                   self.den_t, B, C, self.nr_t)
                Wt = self._view("transform_matrix.0.weight", T_ * D * D, (T_, D, D))
                bt = self._view("transform_matrix.0.bias", T_ * D, (T_, D))
                proj = (self.X, D, 1, self.X.stride(0), Wt, D, 1, D * D, self.Pm, D, self.Pm.stride(0), bt, D, Rt, D, D)
                if side == main:       # the projection rides in the launch of the news encoder's dense layer (encode(extra=...))
                    extra = [self._sgemm_problem(*proj, batch=T_)]
                else:
                    self._sgemm(*proj, batch=T_)
        if T_ == 0 or side != main:
            extra = None
        if news_combined is not None:
            self.plan = plan
            if plan is None:
                self.encode(news_combined, N, nidx=self.nidx, extra=extra)
            else:
                # encode each distinct news once, expand to the slots (dedup.py); everything downstream is unchanged
                assert plan.n_slots == N and plan.n_enc <= self.N_alloc
                self.encode(news_combined, plan.n_enc, nidx=plan.uniq, out=self.Sv, extra=extra)
                T.call("tnr_gather_rows", self.Sv, plan.n_enc, plan.inv, N, D, 1, self.S, self.S.shape[0], 0)
        else:
            assert history.shape[1:] == (U, 2 * L) and candidate.shape[1:] == (C, 2 * L)
            self.plan = plan
            tok = self.tok[:N]
            tok[:B * U].copy_(history.reshape(B * U, 2 * L))
            tok[B * U:].copy_(candidate.reshape(B * C, 2 * L))
            if plan is None:
                self.encode(tok, N, extra=extra)
            else:
                # the token rows fed by the host, de-duplicated as the resident feed is (dedup.py): the row of each distinct news
                # is that of its first slot; the plan's padding entries (no slot, never gathered, zero gradient) are the all-zero
                # pad news, as news_combined[0] is - the encoder then sees what it sees in the resident feed, row for row
                assert plan.n_slots == N and plan.n_enc <= self.N_alloc
                first = plan.order[plan.seg[:plan.n_unique].long()].long()
                self.tok_u = torch.zeros((plan.n_enc, 2 * L), device=self.dev, dtype=tok.dtype)
                self.tok_u[:plan.n_unique] = tok[first]
                self.encode(self.tok_u, plan.n_enc, out=self.Sv, extra=extra)
                T.call("tnr_gather_rows", self.Sv, plan.n_enc, plan.inv, N, D, 1, self.S, self.S.shape[0], 0)
        S = self.S[:Rt]
        g = self.p
        Qu = cfg.Qu
        self._user_forward(S, Rt, 1, self._user_params("student.user_encoder.", 1), hidx, cidx, self.mask, self.epre_u, S[N:],
                           B * D, self.score, self.e_u, self.alpha_u, self.den_u, B, C, self.nr_s)
        if T_ > 0:
            main.wait_stream(side)
        T.call("tnr_kd_score_loss", self.score, self.t_score if T_ else None, self.label, cfg.temperature,
               0.0 if self._ib_on else cfg.coef, self.tw if T_ else None, self.dscore, self.losses, B, C, T_)
        if self._ib_on:
            # dscore holds the distillation part alone (coef = 0 above); this adds the target part over own + eligible foreign
            # candidates and overwrites losses[1]
            T.call("tnr_inbatch_loss", S[N:], D, S[B * U:], D, self.score, self.label, ib["elig"], cfg.coef, self.dscore, ib["dz"],
                   None, ib["per"], self.losses, B, C, D)
        if T_ > 0:
            T.call("tnr_kd_embed_loss", S, self.Pm, self.tw, self.losses[2:], self.dS, self.dP, self.kd_part, B, U, C, D, T_)
        else:
            self.dS[:Rt].zero_()
            self.losses[2:3].zero_()
        return self.losses, self.score[:B]

    def _inbatch_buffers(self):
        """The buffers of the in-batch negatives (forward(inbatch_ids=...)), made on first use for the batch the workspace is laid
        out for and dropped with it (_alloc_workspace): elig (B, W) / first_ws (W) bit words, count (B) int32, dz (B, B C), per (B)."""
        if self._inbatch is None:
            B, M = self.B_alloc, self.B_alloc * self.cfg.C
            W = (M + 31) // 32
            i32 = lambda *s: torch.zeros(s, device=self.dev, dtype=torch.int32)
            f32 = lambda *s: torch.zeros(s, device=self.dev, dtype=torch.float32)
            self._inbatch = dict(elig=i32(B, W), count=i32(B), first_ws=i32(W), dz=f32(B, M), per=f32(B))
        return self._inbatch

    def inbatch_counts(self):
        """count[:B] of the last forward with in-batch negatives: how many foreign slots each impression was ranked against, an
        int32 device tensor (no synchronisation here; the caller's read-back is one)."""
        if not self._ib_on:
            raise RuntimeError("inbatch_counts(): the last forward ran without in-batch negatives")
        return self._inbatch["count"][:self.cur[0]]

    def _user_params(self, first, nm):
        """Stacked parameter views of `nm` user encoders whose first member has prefix `first`."""
        cfg = self.cfg
        D, Qu = cfg.D, cfg.Qu
        v = lambda suffix, per, shape: self._view(first + suffix, nm * per, (nm,) + shape)
        p = dict(pad=v("pad_doc", D, (D,)), w1=v("attn.att_fc1.weight", Qu * D, (Qu, D)), b1=v("attn.att_fc1.bias", Qu, (Qu,)),
                 w2=v("attn.att_fc2.weight", Qu, (Qu,)), b2=v("attn.att_fc2.bias", 1, ()))
        if cfg.nrms_heads:
            p["wqkv"] = v(NRMS_W[0], 3 * D * D, (3 * D, D))
            p["bqkv"] = v(NRMS_B[0], 3 * D, (3 * D,))
        return p

    def _user_forward(self, vec, R, nm, p, hidx, cidx, mask, epre, user, user_stride, score, e, alpha, den, B, C, nr):
        """UserEncoder.forward (model_bert.py:155-176) + scorer bmm for `nm` stacked encoders over the row tables
        vec (nm, R, D): history rows hidx (B,U), candidate rows cidx (B,C)."""
        cfg = self.cfg
        U, D, Qu, ulm = cfg.U, cfg.D, cfg.Qu, int(cfg.user_log_mask)
        if not cfg.nrms_heads:
            if self.fused_user_fwd and D % 8 == 0 and 4 * (64 * (D + 4) + U * Qu + 64 + D) <= 160 * 1024:
                # fc1 inside the kernel: one launch per pass (was: batched fp32 GEMM + split reduce + fc1(pad) pair + this kernel)
                T.call("tnr_user_score_fwd", vec, R, hidx, cidx, mask, p["pad"], p["w1"], p["b1"], p["w2"], p["b2"], ulm, None, None,
                       user, user_stride, score, e, alpha, den, nm, B, U, C, D, Qu)
                return
            sv = vec.stride(0) if vec.dim() == 3 else 0
            self._sgemm(vec, D, 1, sv, p["w1"], D, 1, Qu * D, epre, Qu, B * U * Qu, p["b1"], Qu, B * U, Qu, D, batch=nm)
            epad = None
            if not ulm:        # fc1(pad_doc) once per model instead of once per (impression, model) workgroup
                epad = self.epad_buf[nm]
                self._sgemm(p["pad"], D, 1, D, p["w1"], D, 1, Qu * D, epad, Qu, Qu, p["b1"], Qu, 1, Qu, D, batch=nm)
            T.call("tnr_user_score_fwd", vec, R, hidx, cidx, mask, p["pad"], p["w1"], p["b1"], p["w2"], p["b2"], ulm, epre, epad,
                   user, user_stride, score, e, alpha, den, nm, B, U, C, D, Qu)
            return
        # NRMS (:162-164, :171-173): blend -> self-attention over the clicked news -> additive pooling of its output
        hv, qkv, ctx = nr
        BU = B * U
        T.call("tnr_user_blend_fwd", vec, R, hidx, mask, p["pad"], ulm, hv, nm, B, U, D)
        self._sgemm(hv, D, 1, hv.stride(0), p["wqkv"], D, 1, 3 * D * D, qkv, 3 * D, qkv.stride(0), p["bqkv"], 3 * D, BU, 3 * D, D,
                    batch=nm)
        T.call("tnr_nrms_attn_fwd", qkv, mask, ulm, ctx, ctx.shape[1], nm, B, U, cfg.nrms_heads)
        if C:
            T.call("tnr_gather_rows", vec, R, cidx.reshape(-1), B * C, D, nm, ctx, ctx.shape[1], BU)
        self._sgemm(ctx, D, 1, ctx.stride(0), p["w1"], D, 1, Qu * D, epre, Qu, BU * Qu, p["b1"], Qu, BU, Qu, D, batch=nm)
        # the pooling sees the attention output as it is: no blend (done above), mask only under user_log_mask
        T.call("tnr_user_score_fwd", ctx, ctx.shape[1], self.hpos[:B], self.cpos[:B], mask if ulm else self.ones_mask[:B], p["pad"],
               p["w1"], p["b1"], p["w2"], p["b2"], 1, epre, None, user, user_stride, score, e, alpha, den, nm, B, U, C, D, Qu)

    def _side_stream(self):
        # measured on MI355X (A/B on one box): no gain from a real second stream for the teacher side, so it shares
        # the main one (Engine.teacher_stream = a torch.cuda.Stream to opt in)
        return self.teacher_stream if self.teacher_stream is not None else torch.cuda.current_stream(self.dev)

    def _idx(self, B):
        assert B == self.B_alloc
        return self.hidx, self.cidx

    def total_loss(self):
        """distill + coef*target + emb  (model_bert.py:305) as a device scalar."""
        l = self.losses
        return l[0] + self.cfg.coef * l[1] + l[2]

    # ------------------------------------------------------------------ backward
    def _red_check(self):
        """The batched reductions replay a recorded job table that carries 1 / (loss scale) in its descriptors: when the dynamic
        scale has moved since they were recorded (an fp16 overflow, a growth step) they are recorded afresh."""
        if self._red_ginv != self.ginv:
            self.red.clear()
            self._red_ginv = self.ginv

    def backward(self, after_bucket=None, micro=None):
        """d total_loss / d trainable parameters -> self.flat_g.  after_bucket(i) is called when gradient
        bucket i (0 = heads, then one per layer from the top) is complete (dist.py overlaps its all-reduce).
        micro = (j, K), K > 1: this is micro-batch j of a window of K whose gradients are SUMMED (gradient accumulation; the mean
        is the caller's step(grad_scale = 1 / (world * K))).  Every backward still overwrites flat_g; the sum lives in an fp32
        buffer of its own (_acc_buffer()) and moves by one tnr_grad_accum launch per micro-batch:
          j < K - 1: backward WITHOUT the bucket hook, whatever after_bucket is - no collective starts (DistributedDataParallel's
                     no_sync()) - then acc <- flat_g (j == 0: the accumulator is not read, nothing stale survives) or
                     acc += flat_g over [0, n_train);
          j == K - 1: flat_g += acc - with a hook bucket by bucket, flat_g[s:e] += acc[s:e] on the current stream in front of the
                     caller's hook, so each bucket's collective (ordered behind the current stream by GradSync.launch) carries the
                     window's sum; without one, a single launch over [0, n_train) behind backward (what lies between buckets is
                     zero in both buffers: the same bits on every bucket element).
        flat_g then holds ((g0 + g1) + ...) + g_{K-1}, one correctly rounded fp32 add per element and micro-batch, and the window
        is closed.  j must be the number of micro-gradients held; step() inside a window is an error, accum_reset() drops one.
        fp16: the dynamic loss scale only moves inside step(), so it is one value over the window, and an inf / nan in ANY
        micro-batch's gradient reaches flat_g through the adds: step()'s scan then skips the WHOLE update as one skipped step.
        micro = None or K == 1: the calls, bits and buffers of a backward without it."""
        if micro is not None and int(micro[1]) > 1:
            return self._backward_micro(after_bucket, int(micro[0]), int(micro[1]))
        self._red_check()
        cfg = self.cfg
        B, N, Rt = self.cur
        U, C, D, T_ = cfg.U, cfg.C, cfg.D, cfg.T
        g = self.p
        S, dS = self.S[:Rt], self.dS
        hidx, cidx = self._idx(B)
        rbh = self.red.setdefault(("heads", 0, N if self.plan is None else self.plan.n_enc, after_bucket is None and self.merge_reductions),
                                  _ReduceBatch(self.dev))   # backward_encoder's key
        pend = []                 # fp32 GEMMs that depend on nothing computed below: launched together with the user encoder's
        if T_ > 0:
            self._transform_grads(Rt, rbh, pend)
        # scorer + user encoder
        T.call("tnr_score_bwd", S, cidx, S[N:], self.dscore, dS, dS[N:], B, C, D)
        if self._ib_on:
            ib = self._inbatch_buffers()
            T.call("tnr_inbatch_bwd", ib["dz"], ib["elig"], S[N:], D, S[B * U:], D, dS[N:], dS[B * U:], B, C, D)
        ue = "student.user_encoder."
        Qu, ulm = cfg.Qu, int(cfg.user_log_mask)
        w1u = g(ue + "attn.att_fc1.weight")
        nrms = bool(cfg.nrms_heads)
        # pooling backward: over the history rows themselves, or (NRMS) over the self-attention output
        pv, ph, pm, pu, pd = (S, hidx, self.mask, ulm, dS) if not nrms else \
            (self.nr_s[2][0], self.hpos, self.mask if ulm else self.ones_mask, 1, self.nr_dctx)
        T.call("tnr_user_bwd_pre", pv, ph, pm, g(ue + "pad_doc"), g(ue + "attn.att_fc2.weight"), pu, dS[N:], self.e_u,
               self.alpha_u, self.hv_u, self.dpre_u, self.user_part, B, U, D, Qu)
        # dW1 = dpre^T hv (straight into the gradient) ; dhv = dpre W1      -- fp32 MFMA GEMMs
        self._sgemm_group(pend + [
            self._sgemm_problem(self.dpre_u, 1, Qu, 0, self.hv_u, 1, D, 0, self.grads[ue + "attn.att_fc1.weight"], D, 0, None, 0,
                                Qu, D, B * U, ksplit=self.KS, part=self.sg_part2),
            self._sgemm_problem(self.dpre_u, Qu, 1, 0, w1u, 1, D, 0, self.dhv_u, D, 0, None, 0, B * U, D, Qu)])
        if nrms:
            pd.zero_()
        T.call("tnr_user_bwd_post", self.dhv_u, self.alpha_u, dS[N:], pm, ph, pu, pd, self.user_part, B, U, D, Qu)
        if nrms:
            # self-attention backward (model_bert.py:62-100), then the blend in front of it
            hv, qkv, _ = self.nr_s
            BU = B * U
            T.call("tnr_nrms_attn_bwd", qkv, self.mask, ulm, self.nr_dctx, self.nr_dqkv, B, U, cfg.nrms_heads)
            wqkv = self._view(ue + NRMS_W[0], 3 * D * D, (3 * D, D))
            self._sgemm(self.nr_dqkv, 1, 3 * D, 0, hv, 1, D, 0, self._view(ue + NRMS_W[0], 3 * D * D, (3 * D, D), grad=True), D, 0,
                        None, 0, 3 * D, D, BU, ksplit=self.KS)
            self._c("tnr_colsum", self.nr_dqkv, 3 * D, T.F32, BU, 3 * D, self._view(ue + NRMS_B[0], 3 * D, (3 * D,), grad=True),
                    self.cs_part, 0)
            self._sgemm(self.nr_dqkv, 3 * D, 1, 0, wqkv, 1, D, 0, self.nr_dhv, D, 0, None, 0, BU, D, 3 * D)
            T.call("tnr_user_blend_bwd", self.nr_dhv, self.mask, hidx, ulm, dS, self.user_part[:, 2 * Qu:], self.user_part.shape[1],
                   B, U, D)
        ps = self.user_part.shape[1]
        rbh.add(self.user_part, B, ps, ps, self._view(ue + "attn.att_fc1.bias", ps, (ps,), grad=True))
        if self.plan is None:
            self.backward_encoder(dS[:N], N, after_bucket=after_bucket)
        else:
            p = self.plan
            T.call("tnr_segment_sum_rows", dS, p.order, p.seg, p.n_enc, D, self.dSv)
            self.backward_encoder(self.dSv, p.n_enc, after_bucket=after_bucket)

    def _backward_micro(self, after_bucket, j, K):
        """backward(micro=(j, K)), K > 1 (its docstring)."""
        own = self._clip_owner
        assert 0 <= j < K, "micro = (j, K) needs 0 <= j < K"
        assert j == own._acc_held, "micro-batch %d of %d, but the accumulator holds %d micro-gradients" % (j, K, own._acc_held)
        acc = self._acc_buffer()
        if j < K - 1:
            self.backward()
            T.call("tnr_grad_accum", acc, self.flat_g, self.n_train, 1 if j == 0 else 0)
            own._acc_held = j + 1
            return
        if after_bucket is None:
            self.backward()
            T.call("tnr_grad_accum", self.flat_g, acc, self.n_train, 0)
        else:
            ranges = self.bucket_ranges()

            def fold_then(b):
                s_, e_ = ranges[b]
                T.call("tnr_grad_accum", self.flat_g[s_:e_], acc[s_:e_], e_ - s_, 0)
                after_bucket(b)
            self.backward(after_bucket=fold_then)
        own._acc_held = 0

    def _owned(self, attr, make):
        """State that a mode of the step needs and that no other mode pays for: attribute `attr` of the engine that owns flat_g
        (engines built with share= use the owner's), made by make(owner) on first use.  Never requested, nothing is allocated."""
        own = self._clip_owner
        state = getattr(own, attr)
        if state is None:
            state = make(own)
            setattr(own, attr, state)
        return state

    def _acc_buffer(self):
        """The accumulator of a gradient-accumulation window (backward(micro=...)): fp32, laid out like flat_g, made on first use
        by the engine that owns flat_g; engines built with share= use the owner's.  Never requested, nothing is allocated."""
        return self._owned("_acc", lambda own: torch.zeros_like(own.flat_g))

    def accum_reset(self):
        """Drop a partial accumulation window (an epoch that ends inside one): the next backward(micro=(0, K)) overwrites
        whatever the accumulator holds."""
        self._clip_owner._acc_held = 0

    def _transform_grads(self, Rt, rb, pend=None):
        """dW_i = dP_i^T X_i ; db_i = colsum(dP_i)   (transform_matrix, model_bert.py:278,283).  The bias column sums ride in the
        heads' batched reduction `rb` (flushed in backward_encoder, after the GEMM above has read dP: its first level sums in place)."""
        D, T_ = self.cfg.D, self.cfg.T
        dWt = self._view("transform_matrix.0.weight", T_ * D * D, (T_, D, D), grad=True)
        dbt = self._view("transform_matrix.0.bias", T_ * D, (T_, D), grad=True)
        dwt = (self.dP, 1, D, Rt * D, self.X, 1, D, self.X.stride(0), dWt, D, D * D, None, 0, D, D, Rt)
        if pend is None:
            self._sgemm(*dwt, batch=T_, ksplit=self.KS)
        else:          # the caller groups it with other independent GEMMs (one launch)
            pend.append(self._sgemm_problem(*dwt, batch=T_, ksplit=self.KS))
        for i in range(T_):
            rb.add(self.dP[i], Rt, D, D, dbt[i])

    def backward_encoder(self, dvec, N, acc=0, after_bucket=None, pend=None, **two_parts):
        """NewsEncoder backward for the N sequences of the last encode(): dvec (N,D) fp32 = d loss / d news vectors.
        acc=1 adds to the gradients already in flat_g (second pass over the same parameters, stage 1).
        pend: fp32 GEMM problems of the caller that depend on nothing computed here; they ride in the first grouped launch.
        two_parts: parts, side, group_wgrad of backward_encoder_steps."""
        for _ in self.backward_encoder_steps(dvec, N, acc, after_bucket, pend=pend, **two_parts):
            pass

    def _ln_bwd(self, lnargs, dx_masked, drop, drop_tail, split_row):
        """LayerNorm backward behind a Linear with output dropout `drop`: dx for the residual branch and dx_masked = dx * mask /
        (1 - p), the Linear's output gradient (drop None: off, dx is both).  drop_tail / split_row as in _gemm."""
        if drop is None:
            self._c("tnr_ln_bwd", *lnargs)
        elif drop_tail is not None:
            self._c("tnr_ln_bwd_do_split", *lnargs, dx_masked, drop, drop_tail, split_row)
        else:
            self._c("tnr_ln_bwd_do", *lnargs, dx_masked, drop)

    def backward_encoder_steps(self, dvec, N, acc=0, after_bucket=None, defer=False, split_ffn=False, pend=None, parts=None, side=None,
                               group_wgrad=None):
        """backward_encoder as a generator.  defer=True (stage 1): the weight gradients are not launched but collected in
        self._wg_defer, and the generator yields wherever they have to be on their way - after the pooling head, after every
        trainable layer (and, split_ffn, after its FFN block: the point a gradient bucket completes) - so that a caller running
        two passes over the same parameters in step can launch both passes' contributions to a weight as ONE chained problem.
        parts, side: as in the encode() this backward belongs to; dvec then holds both parts' rows.  Two parts always write
        (acc = 0, no defer), collect a layer's weight gradients if group_wgrad (None: self.group_wgrad) and launch them with one
        round shared by all of them (_wgrad_flush).
        This is the protocol with the caller only - which partial sums are reduced when, where the weight gradients leave, the
        yields and the bucket hook; the kernels are in the block methods below, called in the order of the launches."""
        cfg = self.cfg
        self._red_check()
        parts = parts or [(self, N, 0, 0)]
        two = len(parts) > 1
        assert not two or (acc == 0 and not defer and cfg.pooling == "att")
        self._wg_defer = [] if defer else None
        self._wg = None                    # nothing collected from an earlier, interrupted backward
        group = (self.group_wgrad if group_wgrad is None else group_wgrad) and not defer
        # q / k / v bias: the short-sequence attention backward leaves one partial row per sequence, the long one none (its dqkv
        # columns are summed into ONE row): the parts' rows one behind the other in qkvb_part, one reduction job over all of them
        s = self._parts_state(parts, N, side, acc=acc, qrows=[n if e.cfg.L <= 32 else 1 for e, n, _, _ in parts],
                              gi=self.ginv)        # parameter gradients below the pooling backward: 1 / loss scale on the way out
        s.nblk = T.query("tnr_ln_bwd_blocks", s.M)
        # no bucket hook (one GPU): nothing waits for any bucket, so every partial sum of the backward - heads, layers, embeddings -
        # goes into ONE batched reduction at its end; otherwise a batch per gradient bucket, flushed where the bucket completes
        one = after_bucket is None and self.merge_reductions
        # the recorded reduction tables of one pass (writing or adding) and of two parts never replay each other's
        form = "joint" if two else acc
        rb_heads = self.red.setdefault(("heads", form, s.Ns, one), _ReduceBatch(self.dev))
        batch = lambda *key: rb_heads if one else self.red.setdefault(key, _ReduceBatch(self.dev))
        self._head_bwd_pool(s, dvec, pend, rb_heads)
        if not one or not cfg.trainable_layers:
            rb_heads.flush()
        self._head_bwd_wgrad(s)
        if defer:
            yield "heads"
        if after_bucket:
            after_bucket(0)
        if not cfg.trainable_layers:
            self._wg_defer = None
            return
        dy = self._head_bwd_dgrad(s)
        bucket = 1
        for l in range(cfg.n_layers - 1, self.lo - 1, -1):
            # two gradient buckets per layer, in completion order: the FFN block (names[10:16]) is final after the W1
            # weight gradient, the attention block (names[0:10]) at the end of the layer -- the last all-reduce of a step
            # (attention block of layer lo) is then a third of a layer instead of a whole one
            tr = l in cfg.trainable_layers
            self._wg = [] if (tr and group) else None
            rba, rb = (batch(l, form, s.Ns, "att"), batch(l, form, s.Ns, "ffn")) if tr else (None, None)
            self._ffn_bwd(s, l, dy, rb)
            if tr:
                if not one:
                    rb.flush()
                if defer and split_ffn:
                    yield (l, "ffn")
                if after_bucket:
                    if self._wg is not None:
                        self._wgrad_flush(two)         # the FFN block's two gradients: its bucket goes out now
                    after_bucket(bucket)
                    bucket += 1
            self._att_bwd(s, l, rba)
            if tr:
                if self._wg is not None:               # all four of the layer (two under a bucket hook), before the next layer overwrites their operands
                    self._wgrad_flush(two)
                    self._wg = None
                if defer:
                    yield (l, "att")
                if not one:
                    rba.flush()
            if l > self.lo or cfg.train_embeddings:
                dy = self._qkv_dgrad(l, dy, s.M)
            if tr and after_bucket:
                after_bucket(bucket)
                bucket += 1
        if cfg.train_embeddings:
            assert not two and not defer
            rbe = batch("emb", form, s.Ns)
            self._embed_bwd(dy, N, acc, rbe)
            if not one:
                rbe.flush()
        if one:
            rb_heads.flush()
        if cfg.train_embeddings and after_bucket:
            after_bucket(bucket)           # the embedding block: the last bucket of the step
        self._wg_defer = None

    # The blocks of the backward, in launch order: the news head in the three pieces the driver's flush and yield cut it into, then
    # per layer the FFN block, the attention block and the dgrad into the layer below.  s: the record of _parts_state; rb: the
    # reduction batch of the block's gradient bucket (None for a layer that is not trainable: it only passes the gradient on).
    # Bias and LayerNorm gradients ride along as partial sums - dx column sums from LayerNorm backward, the dgrad epilogue, attention
    # backward - registered with rb.add and reduced by the driver's flush (fixed order).
    def _head_bwd_pool(self, s, dvec, pend, rb):
        """Dense + pooling of the news encoder: dvec -> dnv; attention pooling: -> dpre (fc1's output gradient) and dy2 (the pooled
        sum's share of the last layer's output gradient)."""
        cfg, g, gr, acc, Ns = self.cfg, self.p, self.grads, s.acc, s.Ns
        D, H = cfg.D, cfg.H
        self._sgemm_group(list(pend or []) + [
            self._sgemm_problem(dvec, 1, D, 0, self.nv, 1, H, 0, gr[PFX + "dense.weight"], H, 0, None, 0, D, H, Ns, ksplit=self.KS,
                                beta=float(acc)),
            self._sgemm_problem(dvec, D, 1, 0, g(PFX + "dense.weight"), 1, H, 0, self.dnv, H, 0, None, 0, Ns, H, D,
                                alpha=self.gscale)])      # loss scale enters here
        rb.add(dvec, Ns, D, D, gr[PFX + "dense.bias"], acc)       # column sums; in place, behind the two GEMMs that read dvec
        if cfg.pooling == "att":
            y = self.y_last
            self._per_part(s.parts, s.side, lambda e, n, r0, s0: e._attpool_bwd(
                _from(y, r0), _from(self.e, r0), _from(self.dnv, s0), _from(self.dy2, r0), _from(self.dpre, r0), _from(self.dw2p, s0),
                _from(self.db2p, s0), _from(self.db1p, s0), n))
            rb.add(self.dw2p, Ns, cfg.Qn, cfg.Qn, gr[PFX + "attn.att_fc2.weight"], acc, s.gi)
            rb.add(self.db2p, Ns, 1, 1, gr[PFX + "attn.att_fc2.bias"], acc, s.gi)
            rb.add(self.db1p, Ns, QPAD, QPAD, self._view(PFX + "attn.att_fc1.bias", QPAD, (QPAD,), grad=True), acc, s.gi)

    def _head_bwd_wgrad(self, s):
        if self.cfg.pooling == "att":
            H = self.cfg.H
            self._wgrad(self.dpre, self.y_last, self._view(PFX + "attn.att_fc1.weight", QPAD * H, (QPAD, H), grad=True), s.M, s.acc)

    def _head_bwd_dgrad(self, s):
        """-> dy, the gradient w.r.t. the last layer's output."""
        cfg = self.cfg
        if cfg.pooling == "att":
            self._gemm(self.dpre, self.sh_a1T, self.dy, s.M, res=self.dy2, flags=T.EPI_RES)
        else:
            self._c("tnr_pool_bwd", self.dnv, self.dy, s.N, cfg.L, cfg.H, int(cfg.pooling == "mean"))
        return self.dy

    def _ffn_bwd(self, s, l, dy, rb):
        """Layer l from the second LayerNorm's backward to the W1 weight gradient: dy -> dypre (residual branch), du."""
        cfg, g, gr, acc, gi, M = self.cfg, self.p, self.grads, s.acc, s.gi, s.M
        H, I = cfg.H, cfg.I
        names, sh, a, P = self.lnames[l], self.sh[l], self.act[l - self.lo], self.lpart.get(l)
        tr = rb is not None
        # with dropout behind the two output Linears the LayerNorm backward has two outputs: dx for the residual branch and
        # dx * mask / (1 - p) = the Linear's output gradient (its weight gradient, dgrad and -- through the partials -- bias)
        dF = s.ds(T.DROP_FFN_OUT, l)
        dypre_lin = self.dyprem if dF else self.dypre
        self._ln_bwd((dy, a["ypre"], a["st2"], g(names[14]), self.dypre, None, None, None, (P["ln_part"] if tr else None), M, H),
                     dypre_lin, dF, s.ds2(T.DROP_FFN_OUT, l) if s.two else None, s.M0)
        if tr:
            rb.add(P["ln_part"], s.nblk, 3 * H, 2 * H, self._view(names[14], 2 * H, (2 * H,), grad=True), acc, gi)   # [dgamma | dbeta]
            rb.add(P["ln_part"][2 * H:], s.nblk, 3 * H, H, gr[names[13]], acc, gi)                                 # output.dense.bias
            self._wgrad(dypre_lin, a["g"], gr[names[12]], M, acc)
        fused_cs = tr and M > 128            # the column-sum epilogue needs more than one 128-row strip (a toy batch has less)
        self._gemm(dypre_lin, sh["w2T"], self.du, M, aux=a["u"], flags=T.EPI_MULDGELU | (T.EPI_COLSUM if fused_cs else 0),
                   colsum=P["gcs_part"] if fused_cs else None)
        if tr:
            if fused_cs:
                rb.add(P["gcs_part"], self._q("tnr_gemm_colsum_rows", M), I, I, gr[names[11]], acc, gi)
            else:
                self._c("tnr_colsum", self.du, I, T.BF16, M, I, P["cs_tmp"][:I], self.cs_part, 0)
                rb.add(P["cs_tmp"], 1, I, I, gr[names[11]], acc, gi)
            self._wgrad(self.du, a["h1"], gr[names[10]], M, acc)

    def _att_bwd(self, s, l, rb):
        """Layer l from the W1 dgrad to the QKV weight gradient: du, dypre -> dh1pre (residual branch), dqkv."""
        cfg, g, gr, acc, gi, M = self.cfg, self.p, self.grads, s.acc, s.gi, s.M
        H = cfg.H
        names, sh, a, P = self.lnames[l], self.sh[l], self.act[l - self.lo], self.lpart.get(l)
        tr = rb is not None
        dO = s.ds(T.DROP_ATTN_OUT, l)
        dh1pre_lin = self.dh1prem if dO else self.dh1pre
        self._gemm(self.du, sh["w1T"], self.dh1, M, res=self.dypre, flags=T.EPI_RES)
        self._ln_bwd((self.dh1, a["h1pre"], a["st1"], g(names[8]), self.dh1pre, None, None, None, (P["ln_part1"] if tr else None), M, H),
                     dh1pre_lin, dO, s.ds2(T.DROP_ATTN_OUT, l) if s.two else None, s.M0)
        if tr:
            rb.add(P["ln_part1"], s.nblk, 3 * H, 2 * H, self._view(names[8], 2 * H, (2 * H,), grad=True), acc, gi)
            rb.add(P["ln_part1"][2 * H:], s.nblk, 3 * H, H, gr[names[7]], acc, gi)                               # attention.output.dense.bias
            self._wgrad(dh1pre_lin, a["ctx"], gr[names[6]], M, acc)
        self._gemm(dh1pre_lin, sh["oT"], self.dctx, M)
        qp, qrows = (P["qkvb_part"] if tr else None), s.qrows

        def attn(e, n, r0, s0):
            q0 = qrows[0] if r0 else 0             # the part's first row of qkvb_part
            dqkv = _from(self.dqkv, r0)
            if not e._attn_bwd(_from(a["qkv"], r0), _from(a["ctx"], r0), e.act[l - e.lo]["lse"], _from(self.dctx, r0), dqkv,
                               _from(qp, q0) if tr else None, n, e._dsite(T.DROP_PROB, l)) and tr:
                e._c("tnr_colsum", dqkv, 3 * H, T.BF16, n * e.cfg.L, 3 * H, qp[q0], e.cs_part, 0)
        self._per_part(s.parts, s.side, attn)
        if tr:
            rb.add(qp, sum(qrows), 3 * H, 3 * H, self._view(names[3], 3 * H, (3 * H,), grad=True), acc, gi)
            self._wgrad(self.dqkv, self.x_in[l], self._view(names[0], 3 * H * H, (3 * H, H), grad=True), M, acc)

    def _qkv_dgrad(self, l, dy, M):
        """The gradient handed to the layer below: dqkv, dh1pre -> whichever of dy / dy2 layer l's own input gradient `dy` is not."""
        nxt = self.dy2 if dy is self.dy else self.dy
        self._gemm(self.dqkv, self.sh[l]["qkvT"], nxt, M, res=self.dh1pre, flags=T.EPI_RES)
        return nxt

    def _embed_bwd(self, dy, n_seq, acc, rb):
        """BertEmbeddings backward (tnlrv3/modeling.py:153-178) for the sequences of the last encode(): dy (n_seq L, H) 16-bit =
        gradient w.r.t. the embedding output at the loss scale -> the gradients of the three tables and of the embedding LayerNorm.
        tnr_embed_ln_bwd recomputes the forward's rows and leaves fp32 dx at the true scale; the word rows are a fixed-order
        scatter-sum of dx keyed by token id (row 0 = padding_idx of :138 never gets one), the position rows the column sums of the
        (n_seq, L H) view, the token-type row 0 the column sums of those.  Keys and order are integer index preparation on the
        device (like _pos_ids): the token ids of the ENCODED rows - after de-duplication the distinct news, in resident mode
        gathered from the table by nidx - through a stable sort."""
        cfg, g, gr = self.cfg, self.p, self.grads
        L, H = cfg.L, cfg.H
        E_ = BERT + "embeddings."
        tok, nidx, n_enc = self._emb_src
        assert n_enc == n_seq and self.drop_cur is None, "embedding backward: no dropout site, one part"
        M = n_seq * L
        args = (n_seq, L, H, dy, g(E_ + "word_embeddings.weight"), g(E_ + "position_embeddings.weight"),
                g(E_ + "token_type_embeddings.weight"), g(E_ + "LayerNorm.weight"), cfg.ln_eps, self.ginv, self.dx_emb, self.emb_part,
                None, None)
        if nidx is None:
            self._c("tnr_embed_ln_bwd", tok, *args)
            ids = tok[:n_seq, :L]
        else:
            self._c("tnr_embed_ln_bwd_indexed", tok, nidx, *args)
            ids = tok[nidx[:n_seq].long(), :L]
        nblk = T.query("tnr_embed_ln_bwd_blocks", M)
        rb.add(self.emb_part, nblk, 2 * H, 2 * H, self._view(E_ + "LayerNorm.weight", 2 * H, (2 * H,), grad=True), acc, self.ginv)
        keys, order = torch.sort(ids.reshape(-1).to(torch.int32), stable=True)
        gw = gr[E_ + "word_embeddings.weight"]
        if not acc:
            gw.zero_()                     # rows no token of this step names keep no stale gradient
        T.call("tnr_scatter_sum_rows", self.dx_emb, M, H, keys, order.to(torch.int32), 0, gw, cfg.vocab, 1)
        gp = gr[E_ + "position_embeddings.weight"]
        self._c("tnr_colsum", self.dx_emb, L * H, T.F32, n_seq, L * H, gp, self.emb_cs_part, acc)        # rows >= L get nothing
        # token-type row 0 = the sum of all dx rows = the column sums of this step's position rows (not of gp: under acc it holds more)
        if acc:
            self._c("tnr_colsum", self.dx_emb, H, T.F32, M, H, gr[E_ + "token_type_embeddings.weight"], self.emb_cs_part, 1)
        else:
            self._c("tnr_colsum", gp, H, T.F32, L, H, gr[E_ + "token_type_embeddings.weight"], self.emb_cs_part, 0)

    def grad(self, name):
        """Gradient of a trainable parameter (a view into flat_g; the fp16 loss scale never reaches it)."""
        return self.grads[name]

    def bucket_ranges(self):
        """Contiguous [start, end) slices of flat_g in the order their gradients complete."""
        out = [(self.off(PFX + ("attn.att_fc1.weight" if self.cfg.pooling == "att" else "dense.weight")), self.n_train)]
        for l in sorted(self.cfg.trainable_layers, reverse=True):
            names = layer_param_order(l)
            a0, f0 = self.off(names[0]), self.off(names[10])
            e = self.off(names[-1]) + self.slot[names[-1]][2]
            out.append((f0, _rup(e, 64)))          # FFN block: intermediate.dense .. output.LayerNorm
            out.append((a0, f0))                   # attention block: q/k/v .. attention.output.LayerNorm
        if self.cfg.train_embeddings:              # the embedding block (tables + LayerNorm) completes last
            last = BERT + "embeddings.LayerNorm.bias"
            out.append((self.off(BERT + "embeddings.word_embeddings.weight"), _rup(self.off(last) + self.slot[last][2], 64)))
        return out

    # ------------------------------------------------------------------ optimiser
    def _clip_buffers(self):
        """State of global-norm clipping, made on first use by the engine that owns flat_g (engines built with share= use it):
        the scanned slices (bucket_ranges()) with the offset of each one's partial sums, the partial buffer sized through
        tnr_grad_sumsq_parts, the two floats (coefficient, norm) on the device and a pinned ring for their read-back."""
        def make(own):
            slices, off = [], 0
            for s_, e_ in own.bucket_ranges():
                slices.append((s_, e_, off))
                off += T.query("tnr_grad_sumsq_parts", e_ - s_)
            return SimpleNamespace(slices=slices, n_part=off, part=torch.zeros(off, dtype=torch.float32, device=own.dev),
                                   clip=torch.zeros(2, dtype=torch.float32, device=own.dev),
                                   ring=torch.zeros(8, 2, dtype=torch.float32).pin_memory(), count=0, last=None)
        return self._owned("_clip_state", make)

    @staticmethod
    def _read_back(st, src):
        """Queue a copy of `src` into the next slot of st.ring (pinned, 8 slots) and an event behind it, and keep (host, event)
        in st.last: the step never waits for a figure it only reports."""
        host = st.ring[st.count % 8]
        st.count += 1
        host.copy_(src, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        st.last = (host, ev)

    @staticmethod
    def _last_read_back(st):
        """The host copy _read_back queued last, once its event has completed (nothing else is waited for); None before the first."""
        if st is None or st.last is None:
            return None
        host, ev = st.last
        ev.synchronize()
        return host

    def grad_norm(self):
        """(total_norm, coef) of the last clipped step: the norm of grad_scale * (the reduced gradient) and the coefficient the
        update multiplied it by.  Read back asynchronously: step() queued a 8-byte copy into pinned memory and an event behind its
        commit kernel, and this waits for that event only - neither it nor step() drains the device.  None before the first
        clipped step.  fp16: the values of a step the overflow guard skipped are meaningless."""
        host = self._last_read_back(self._clip_owner._clip_state)
        return None if host is None else (float(host[1]), float(host[0]))

    def _decay_bits(self):
        """The decay map (decay_words of the slot table) on the device, made on first use by the engine that owns flat_g; engines
        built with share= use the owner's."""
        return self._owned("_decay_map", lambda own: torch.from_numpy(decay_words(own.slot, own.n_train).view(np.int32)).to(own.dev))

    def _lamb_buffers(self):
        """State of step(lamb=True), made on first use by the engine that owns flat_g (engines built with share= use it, so a
        shared slot table yields ONE chunk table): lamb_chunks of the slot table on the host and on the device, two fp32
        partials per chunk, the trust table (trust, ||w||, ||u|| per tensor) and a pinned ring for its read-back."""
        def make(own):
            names, chunks, tensors = lamb_chunks(own.slot, own.n_train)
            ch, tn = torch.from_numpy(chunks).contiguous(), torch.from_numpy(tensors).contiguous()
            nt = len(names)
            return SimpleNamespace(
                names=names, chunks_host=ch, tensors_host=tn, chunks=ch.to(own.dev), tensors=tn.to(own.dev), n_chunks=len(chunks),
                n_tensors=nt, firsts=chunks[:, 0].astype(np.int64), adapted=[i for i in range(nt) if tensors[i, 2]],
                part=torch.zeros(2 * len(chunks), dtype=torch.float32, device=own.dev),
                trust=torch.zeros(3 * nt, dtype=torch.float32, device=own.dev),
                ring=torch.zeros(8, 3 * nt, dtype=torch.float32).pin_memory(), count=0, last=None)
        return self._owned("_lamb_state", make)

    def trust_ratios(self):
        """{name: (trust, ||w||, ||u||)} of the adapted tensors (the decay set) at the last step(lamb=True): the ratio the update
        of that tensor was multiplied by and the two norms it came from (w before the update).  Read back like grad_norm(): step()
        queued a copy into pinned memory and an event behind its last launch, and this waits for that event only.  None before
        the first such step.  fp16: a step the overflow guard skipped leaves the table of the step before it."""
        ls = self._clip_owner._lamb_state
        host = self._last_read_back(ls)
        if host is None:
            return None
        nt = ls.n_tensors
        return {ls.names[i]: (float(host[i]), float(host[nt + i]), float(host[2 * nt + i])) for i in ls.adapted}

    def _ema_buffer(self):
        """The average of flat[True] (step(ema_decay > 0)): fp32, laid out like flat[True], made on first use by the engine that
        owns flat[True] as a copy of the parameters as they are now, on the current stream (the first step with the average on
        calls this before its update); engines built with share= use the owner's."""
        def make(own):
            own.ema_updates = 0
            return own.flat[True].clone()
        return self._owned("_ema", make)

    @property
    def ema_updates(self):
        """How many updates the average has taken (settable: a checkpoint's count).  Steps the fp16 guard skipped are taken out as
        the host hears of them, like Adam's count: exact once the scaler is drained."""
        own = self._clip_owner
        return own._ema_updates[0] - (own.scaler.skipped - own._ema_updates[1])

    @ema_updates.setter
    def ema_updates(self, n):
        own = self._clip_owner
        own._ema_updates = [int(n), own.scaler.skipped]

    def ema_state_dict(self):
        """The reference-keyed state dict of the AVERAGED model: trainable parameters from the average, frozen ones (teachers,
        frozen layers, embeddings) from flat[False], exactly as state_dict() has them.  None if no step ever ran with ema_decay
        and nothing was loaded."""
        ema = self._clip_owner._ema
        if ema is None:
            return None
        out = {}
        for k, v in self.params.items():
            tr, o, n, shp = self.slot[k]
            out[k] = (ema[o:o + n].view(shp) if tr else v).detach().clone()
        return out

    def load_ema_state_dict(self, sd):
        """Write the trainable slots of the average from a state dict with the reference's keys (ema_state_dict()'s), making the
        buffer if there is none yet (what lies between the slots starts as the parameters' gaps).  Frozen keys are ignored: they
        have no average.  load_state_dict() never touches the average."""
        ema = self._ema_buffer()
        for k, (tr, o, n, shp) in self.slot.items():
            if not tr:
                continue
            if k not in sd:
                raise KeyError("missing key: %s" % k)
            v = sd[k] if isinstance(sd[k], torch.Tensor) else torch.as_tensor(sd[k])
            if tuple(v.shape) != tuple(shp):
                raise ValueError("%s: shape %s != %s" % (k, tuple(v.shape), shp))
            ema[o:o + n].view(shp).copy_(v.to(self.dev, torch.float32))

    def optimizer_state_dict(self):
        """Everything the fused update carries from one step to the next, as CPU data (optstate.py, format 1): Adam's moments per
        trainable key (exp_avg / exp_avg_sq / max_exp_avg_sq = adam_m / adam_v / adam_vmax, shaped like the parameter; vmax is all
        zeros after plain Adam), "step" = the updates TAKEN (the count the bias corrections, the schedule and ema_warmup follow),
        the fp16 loss scaler (host fields and the four guard words), the average's update count and the dropout call counter.
        Under fp16 the scaler is drained first, as at every epoch end, so step_count, skipped and the multiplier are final.
        Not inside an accumulation window.  No kernel is launched (device-to-host copies only) and no device buffer changes.
        Parameters and the average travel in state_dict() / ema_state_dict(); gradients, the accumulator, the clip and decay
        buffers and the 16-bit copies are outputs or pure functions of the slot table.  Engines built with share= forward to the
        owner of the flat buffers."""
        own = self._clip_owner
        if own is not self:
            return own.optimizer_state_dict()
        assert self._acc_held == 0, "optimizer_state_dict() inside an accumulation window"
        sc, scd = self.scaler, None
        if sc.enabled:
            sc.drain(self)
            scd = {f: getattr(sc, f) for f in optstate.SCALER_FIELDS}
            scd["guard"] = [int(x) for x in sc.guard.cpu().tolist()]
        return optstate.make(self.dtype, self.step_count, optstate.unpack(self.slot, self.adam_m, self.adam_v, self.adam_vmax), scd,
                             None if self._ema is None else self.ema_updates, int(self.drop_calls))

    def load_optimizer_state_dict(self, osd):
        """Continue from optimizer_state_dict()'s data: call it AFTER load_state_dict() (which resets the scaler) and
        load_ema_state_dict().  Outstanding scaler answers are consumed; adam_m / adam_v / adam_vmax are rewritten whole (zero
        between the slots); then the scaler's host fields and guard words (guard[1] and scaler.skipped agree: the kernels compute
        guard[1] - known_skips), step_count, the average's update count (its setter reads scaler.skipped) and the dropout call
        counter, in that order.  Parameters, 16-bit copies, the average's buffer, flat_g and the accumulator are not touched, and
        no kernel is launched (host-to-device copies only).  ValueError: unknown format, a state saved under the other 16-bit
        type, a shape that differs; KeyError: a trainable key that is missing, a key that is not trainable here.  Nothing is
        written before those checks have passed."""
        own = self._clip_owner
        if own is not self:
            return own.load_optimizer_state_dict(osd)
        assert self._acc_held == 0, "load_optimizer_state_dict() inside an accumulation window"
        optstate.check_header(osd, self.dtype)
        m, v, vmax = optstate.pack(self.slot, self.n_train, osd["state"])
        sc = self.scaler
        if sc.enabled:
            saved = osd.get("scaler")
            if saved is None:
                raise ValueError("optimiser state: no scaler state, but this engine runs fp16 with the dynamic loss scale")
            if int(saved["guard"][1]) != int(saved["skipped"]):
                raise ValueError("optimiser state: guard[1] = %d but skipped = %d (the state was not saved drained)"
                                 % (int(saved["guard"][1]), int(saved["skipped"])))
            sc.drain(self)
        self.adam_m.copy_(m)
        self.adam_v.copy_(v)
        self.adam_vmax.copy_(vmax)
        if sc.enabled:
            sc.mult, sc.clean, sc.run_of_skips = float(saved["mult"]), int(saved["clean"]), int(saved["run_of_skips"])
            sc.skipped, sc.stamp = int(saved["skipped"]), int(saved["stamp"])
            sc.guard.copy_(torch.tensor([int(x) for x in saved["guard"]], dtype=torch.int32))
        self.step_count = int(osd["step"])
        if osd.get("ema_updates") is not None:
            self.ema_updates = int(osd["ema_updates"])
        self.drop_calls = int(osd["dropout_calls"])

    def _rate_ranges(self, lr, lr_bert, lr_news_head):
        """[(lo, hi, rate)] over flat[True], a pure function of the slot table and the three rates: the BERT layers at lr_bert, the
        news encoder's pooling + dense at lr_news_head, the user encoders / transform matrices at lr (None: lr).  Neighbours with
        one rate are one range, i.e. one launch."""
        head0 = self.slot[PFX + ("attn.att_fc1.weight" if self.cfg.pooling == "att" else "dense.weight")][1]   # end of the BERT layers
        _, o, n, _ = self.slot[PFX + "dense.bias"]
        rest0 = min(_rup(o + n, 64), self.n_train)   # user encoders / transform matrices start here
        lb = lr if lr_bert is None else lr_bert
        lh = lr if lr_news_head is None else lr_news_head
        ranges = []
        for lo_, hi_, rate in ((0, head0, lb), (head0, rest0, lh), (rest0, self.n_train, lr)):
            if ranges and ranges[-1][2] == rate and ranges[-1][1] == lo_:
                ranges[-1] = (ranges[-1][0], hi_, rate)
            elif hi_ > lo_:
                ranges.append((lo_, hi_, rate))
        return ranges

    def _gather(self, sync, guard, stamp, max_grad_norm, grad_scale, lamb_on):
        """The gather phase of step(): bring in the WHOLE reduced gradient and leave on the device what the update reads of it -
        the guard word (guard is not None: fp16) and the clip coefficient (max_grad_norm is not None) - before any slice is
        updated.  Returns the clip state (None without clip).  A sync whose collectives have landed is waited for whole
        (sync.wait()) in front of the first scan; with collectives in flight each bucket is scanned behind its own wait_bucket, in
        completion order, so the scans hide under the collectives still in flight.
        clip: the gradient is ALWAYS scanned slice by slice over bucket_ranges() in that order (tnr_grad_sumsq_scan, which under
        fp16 is the overflow guard's scan as well), so the coefficient's bits do not depend on whether the step ran
        data-parallel; then tnr_grad_nonfinite_commit (fp16) and tnr_grad_clip_commit.
        guard without clip: the whole gradient decides - identically on every rank, since inf / nan survive the all-reduce.
        Bucketed, tnr_grad_nonfinite_scan per bucket of sync.ranges as given (what lies between buckets are alignment gaps, zero
        gradients), then the one-thread tnr_grad_nonfinite_commit: only the last bucket's scan, the commit and the update itself
        (79 us at the headline) stay behind the last collective.  Otherwise the fused tnr_grad_nonfinite over everything.
        neither (bf16 LAMB; bf16 without a pending sync): the waits alone.
        Under clip and under LAMB a pending sync's buckets must be bucket_ranges() (the slices of the clip state; the order a
        tensor's norm may rely on)."""
        cs = self._clip_buffers() if max_grad_norm is not None else None
        bucketed = sync is not None and sync.pending
        if bucketed:
            if cs is not None:
                assert [tuple(r) for r in sync.ranges] == [(s_, e_) for s_, e_, _ in cs.slices], "sync buckets are not bucket_ranges()"
            elif lamb_on:
                assert [tuple(r) for r in sync.ranges] == [tuple(r) for r in self.bucket_ranges()], "sync buckets are not bucket_ranges()"
        elif sync is not None:
            sync.wait()
        if cs is not None:
            for b, (s_, e_, off) in enumerate(cs.slices):
                if bucketed:
                    sync.wait_bucket(b)
                T.call("tnr_grad_sumsq_scan", self.flat_g[s_:e_], e_ - s_, cs.part[off:], guard, stamp)
            if guard is not None:
                T.call("tnr_grad_nonfinite_commit", guard, stamp)
            T.call("tnr_grad_clip_commit", cs.part, cs.n_part, float(max_grad_norm), grad_scale, cs.clip)
        elif bucketed:
            for b, (s_, e_) in enumerate(sync.ranges):
                sync.wait_bucket(b)
                if guard is not None:
                    T.call("tnr_grad_nonfinite_scan", self.flat_g[s_:e_], e_ - s_, guard, stamp)
            if guard is not None:
                T.call("tnr_grad_nonfinite_commit", guard, stamp)
        elif guard is not None:
            T.call("tnr_grad_nonfinite", self.flat_g, self.n_train, guard, stamp)
        return cs

    def step(self, lr, grad_scale=1.0, beta1=0.9, beta2=0.999, eps=1e-8, lr_bert=None, amsgrad=True, lr_news_head=None, sync=None,
             max_grad_norm=None, weight_decay=0.0, warmup_steps=0, lr_decay_steps=0, ema_decay=None, ema_warmup=False, lamb=False):
        """torch.optim.Adam(amsgrad=True).step() (run.py:134,195) + refresh of the 16-bit weight copies.
        Phases, each written once and run in this order.  Setup: flags, the scaler's poll and stamp, step_count, the schedule's
        and the average's three candidates, the rate ranges (_rate_ranges).  Gather (_gather): the whole reduced gradient, the
        guard word and the clip coefficient left on the device.  Update: the Adam family, one launch per rate range, or LAMB
        (norms, commit, one launch per rate range).  Afterwards: scaler.record, the clip read-back, the trust read-back
        (_read_back), refresh_shadows.  One mode has no gather: bf16 with collectives in flight and neither clip nor LAMB needs no
        whole gradient, and its update runs slice by slice behind each wait_bucket, then over what lies outside the buckets.
        lr_bert / lr_news_head: learning rates of the encoder layers / of the news encoder's pooling + dense when they
        differ (PLM-NR/run.py:104-106: {'params': pretrained, 'lr': pretrain_lr}, {'params': rest, 'lr': lr}; the notebooks
        use 1e-6 for bert_model and 1e-5 for the rest).  amsgrad=False: plain Adam (Post-train_KD.ipynb cell 18).
        sync: a dist.GradSync with all-reduces in flight -- the update then runs bucket by bucket in completion order, each
        slice behind its own collective only (elementwise optimiser: the same bits as one launch over everything).
        max_grad_norm > 0: torch.nn.utils.clip_grad_norm_(all trainable parameters, max_grad_norm) on grad_scale * flat_g, i.e.
        AFTER the data-parallel reduction (a clip_grad_norm_ between backward() and step() would see the un-reduced gradient) and
        on the device: ONE norm over everything trainable, whatever the learning-rate ranges.  The gradient is then ALWAYS scanned
        slice by slice over bucket_ranges(), with a pending sync each bucket behind its own wait_bucket (_gather has the call
        sequence), so the coefficient's bits do not depend on whether the step ran data-parallel; then the update of every rate
        range through tnr_amsgrad_step_clipped.  A global norm needs the whole gradient first, so under bf16 this REPLACES the
        bucket-by-bucket update: the update waits for the last bucket, as fp16's always does.  grad_norm() reads the result back.
        None or <= 0: off - the calls, kernels, bits and buffers of a step without it.
        weight_decay > 0: torch.optim.AdamW's decoupled decay - p *= 1 - lr_k weight_decay, then the update on the undecayed
        (clipped) gradient - for the 2-D `.weight`s outside LayerNorm (decays(): biases, LayerNorm parameters, pad_doc and
        alignment gaps are exempt; with train_embeddings the three embedding tables decay), ONE value for every rate range; the
        decay set lives on the device as one bit per element of the flat buffer (decay_words, made once by the owner of flat_g).
        warmup_steps = W, lr_decay_steps = T: every rate is multiplied by lr_schedule(u, W, T), u = the number of updates TAKEN
        before this one, from the step_count the bias corrections use: under fp16 the kernel gets the rates of u, u - 1, u - 2
        beside the three bias corrections and picks by the skips the host has not accounted for, so a skipped step advances
        neither Adam's count nor the schedule and decays nothing.  The position is optimiser state: optimizer_state_dict() saves
        it as "step" beside m, v and vmax (run.py --save_optimizer True / --resume True).  With any of the three on, every range / bucket launch goes through tnr_adamw_step (clip and guard as before);
        all off (None, 0): the calls, kernels, bits and buffers of a step without them.
        ema_decay = d in (0, 1]: an exponential moving average of the trainable parameters, ema <- d ema + (1 - d) p_new inside the
        update kernel (torch.optim.swa_utils.AveragedModel with get_ema_multi_avg_fn(d)), in an fp32 buffer laid out like flat[True]
        that the owner of flat[True] makes on the first such step as a copy of the parameters BEFORE that update (engines built
        with share= use it).  Every range / bucket launch then goes through tnr_adamw_step_ema on all three paths (elementwise:
        the same bits on each).  ema_warmup: d(u) = min(d, (1 + u) / (10 + u)) (ema_decay_at), u = the updates TAKEN before this
        one, from the step_count the bias corrections use - the kernel gets the weights 1 - d of u, u - 1, u - 2 and picks as it
        picks the rates, and a step the fp16 guard skips leaves the average's bits.  Data parallelism has nothing to communicate:
        the average is an elementwise function of parameters that are identical on every rank, so it is identical too.
        ema_state_dict() / load_ema_state_dict() read and write it; load_state_dict() does not touch it.  None or <= 0: off - the
        calls, kernels, bits and buffers of a step without it.
        Gradient accumulation (backward(micro=(j, K))) adds nothing here but an assertion: the window's mean is grad_scale =
        1 / (world * K) on the summed flat_g, so the clip norm, the guard, the decay, the schedule and the average see what torch
        shows them after K backwards of loss / K, with no extra pass.
        lamb=True: LAMB (You et al., Algorithm 2; the contract: include/tnr_hip.h).  The moments are Adam's /
        AMSGrad's; per tensor of the slot table u = (m / c1) / (sqrt(vhat) / sqrt(c2) + eps) + weight_decay * w on the decay set
        (u without the decay term elsewhere), and w <- w - lr_k * trust * u with trust = ||w|| / ||u|| for the tensors of the
        decay set (whatever weight_decay is; 1 if either norm is 0) and 1 for every other tensor: biases, LayerNorm parameters
        and pad_doc take the plain Adam update.  weight_decay is then this COUPLED decay, not AdamW's.  A tensor's norm needs its
        whole gradient, so with a pending sync the step waits for every bucket first, in bucket_ranges() order, scanning each as
        it lands when clip or the guard is on (the scans and commits are today's); then tnr_lamb_norms over the whole chunk table,
        tnr_lamb_commit, tnr_lamb_step per rate range.  No tnr_amsgrad_step* / tnr_adamw_step* call is made, no new optimiser state
        exists (optimizer_state_dict() is unchanged) and nothing is communicated: the trust ratios are a deterministic function of
        buffers that are identical on every rank.  trust_ratios() reads the result back.  False / None: off - the calls, kernels,
        bits and buffers of a step without it, nothing allocated."""
        assert self._clip_owner._acc_held == 0, "step() inside an accumulation window"
        lamb_on = bool(lamb)
        clip_on = max_grad_norm is not None and max_grad_norm > 0
        ema_d = float(ema_decay or 0.0)
        ema_on = ema_d > 0.0
        assert ema_d <= 1.0, "ema_decay must not exceed 1"
        wd = float(weight_decay or 0.0)
        W_, Td = int(warmup_steps or 0), int(lr_decay_steps or 0)
        assert wd >= 0.0 and W_ >= 0 and Td >= 0, "weight_decay, warmup_steps and lr_decay_steps must not be negative"
        sched_on = W_ > 0 or Td > 0
        adamw_on = wd > 0.0 or sched_on
        sc = self.scaler
        guard, stamp = None, 0
        if sc.enabled:
            used = sc.mult                   # what this step's backward ran with
            sc.poll(self)                    # overflows of steps two or more back: scale halved, Adam's count corrected
            sc.stamp += 1
            guard, stamp = sc.guard, sc.stamp
        self.step_count += 1
        if adamw_on:
            # candidates k = 0, 1, 2: t_k = max(step_count - k, 1) updates taken including this one (the launcher's t_k)
            mult = [lr_schedule(max(self.step_count - k, 1) - 1, W_, Td) for k in range(3)]
            wbits = self._decay_bits() if wd > 0.0 and not lamb_on else None
        elif ema_on or lamb_on:
            mult, wbits = (1.0, 1.0, 1.0), None
        self.lr_scale = mult[0] if sched_on else None
        if ema_on:
            ema = self._ema_buffer()                 # first time: the parameters as they are before this update
            self.ema_updates += 1
            # formed in double, rounded once (by the float argument)
            ema_w = [1.0 - ema_decay_at(max(self.step_count - k, 1) - 1, ema_d, ema_warmup) for k in range(3)]
        ranges = self._rate_ranges(lr, lr_bert, lr_news_head)

        def launch(lo_, hi_, rate):
            if hi_ > lo_:
                args = (self.flat[True][lo_:hi_], self.flat_g[lo_:hi_], self.adam_m[lo_:hi_], self.adam_v[lo_:hi_],
                        self.adam_vmax[lo_:hi_] if amsgrad else None, hi_ - lo_, self.step_count, rate, beta1, beta2, eps, grad_scale)
                if ema_on:
                    T.call("tnr_adamw_step_ema", *args[:7], rate * mult[0], rate * mult[1], rate * mult[2], beta1, beta2, eps,
                           grad_scale, wd, wbits, lo_, guard, stamp, sc.skipped if guard is not None else 0,
                           cs.clip if clip_on else None, ema[lo_:hi_], ema_w[0], ema_w[1], ema_w[2])
                elif adamw_on:
                    T.call("tnr_adamw_step", *args[:7], rate * mult[0], rate * mult[1], rate * mult[2], beta1, beta2, eps, grad_scale,
                           wd, wbits, lo_, guard, stamp, sc.skipped if guard is not None else 0, cs.clip if clip_on else None)
                elif clip_on:
                    T.call("tnr_amsgrad_step_clipped", *args, guard, stamp, sc.skipped if guard is not None else 0, cs.clip)
                elif guard is None:
                    T.call("tnr_amsgrad_step", *args)
                else:
                    T.call("tnr_amsgrad_step_guarded", *args, guard, stamp, sc.skipped)

        # bf16 with collectives in flight and nothing that needs the whole gradient first: the update itself runs bucket by bucket
        by_bucket = not (lamb_on or clip_on) and guard is None and sync is not None and bool(sync.pending)
        ls = self._lamb_buffers() if lamb_on else None
        cs = None if by_bucket else self._gather(sync, guard, stamp, max_grad_norm if clip_on else None, grad_scale, lamb_on)
        if by_bucket:
            done = []
            for b, (s_, e_) in enumerate(sync.ranges):       # completion order of backward = launch order of the all-reduces
                sync.wait_bucket(b)
                for lo_, hi_, rate in ranges:
                    launch(max(lo_, s_), min(hi_, e_), rate)
                done.append((s_, e_))
            pos = 0                                          # anything outside the buckets (alignment gaps: zero gradients)
            for s_, e_ in sorted(done) + [(self.n_train, self.n_train)]:
                for lo_, hi_, rate in ranges:
                    launch(max(lo_, pos), min(hi_, s_), rate)
                pos = max(pos, e_)
        elif lamb_on:
            known = sc.skipped if guard is not None else 0
            clip_ = cs.clip if clip_on else None
            vmax_ = self.adam_vmax if amsgrad else None
            T.call("tnr_lamb_norms", self.flat[True], self.flat_g, self.adam_m, self.adam_v, vmax_, self.n_train, ls.chunks,
                   ls.chunks_host, ls.n_chunks, ls.n_tensors, self.step_count, beta1, beta2, eps, grad_scale, wd, guard, stamp,
                   known, clip_, ls.part)
            T.call("tnr_lamb_commit", ls.part, ls.n_chunks, ls.tensors, ls.tensors_host, ls.n_tensors, ls.trust, guard, stamp)
            for lo_, hi_, rate in ranges:
                c0, c1 = int(np.searchsorted(ls.firsts, lo_)), int(np.searchsorted(ls.firsts, hi_))
                if c1 > c0:      # a rate range starts and ends where a storage group does, so no chunk straddles its bounds
                    T.call("tnr_lamb_step", self.flat[True], self.flat_g, self.adam_m, self.adam_v, vmax_, self.n_train,
                           ls.chunks[c0:c1], ls.chunks_host[c0:c1], c1 - c0, ls.n_tensors, self.step_count, rate * mult[0],
                           rate * mult[1], rate * mult[2], beta1, beta2, eps, grad_scale, wd, guard, stamp, known, clip_, ls.trust,
                           ema if ema_on else None, *(ema_w if ema_on else (0.0, 0.0, 0.0)))
        else:
            for lo_, hi_, rate in ranges:
                launch(lo_, hi_, rate)
        if guard is not None:
            sc.record(used)
        if clip_on:
            self._read_back(cs, cs.clip)
        if lamb_on:
            self._read_back(ls, ls.trust)
        self.refresh_shadows(all_layers=False)
