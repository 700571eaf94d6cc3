"""Stage-1 knowledge distillation (title/body matching post-training) on the HIP engine.

Mirrors DistillModel.forward of the reference's Post-train_KD.ipynb (cells 12-14):
    body_vec  = news_encoder(body)                       (B, D)        bodies of up to 512 tokens
    title_vec = news_encoder(title)                      (B, 1+K, D)
    score     = bmm(title_vec, body_vec)                 (B, 1+K)
    loss      = CE(score, label) + kd_ce(mixed teacher scores, tau=1) + sum_t w_t * (MSE_title + MSE_body)
with per-sample teacher weights w = softmax(-CE(teacher score)).  The list*tensor product the notebook writes
for the weighted sum is evaluated as the stacked product it intends (oracle/newsrec_oracle.py:distill_fwd pins
that reading against the notebook's own modules).

One model, two sequence lengths: two Engine instances share parameters / gradients / optimiser state / 16-bit
weight copies and own their workspaces.
JOINT passes (`Stage1Engine.joint`, the default, with dropout or without): a Linear, a LayerNorm and a weight gradient act on token
rows one by one, so the body pass's rows are laid directly BEHIND the title pass's in every per-token buffer and each of them is
ONE launch over M = N Lt + B Lb rows instead of one per pass (8 896 rows at 30 / 128, 24 064 at 24 / 512: tile orders large enough
for the persistent 256-wide kernels); only what depends on the sequence length - embeddings, attention, pooling - still runs per
pass, on its row range (one stream: `joint_streams` puts the body's on a second one, measured slower).  A layer's four weight
gradients leave in ONE grouped persistent launch whose units share one round (Engine._wgrad_flush, shared_round).  There is no layer
loop here: Engine.encode and Engine.backward_encoder_steps run the engine's per-block methods over a list of parts of the host
engine's buffers, one for a single pass, and this class only hands them two - [(title, N, 0, 0), (body, B, N Lt, N)], the title
engine as host (`_parts`).
The per-pass forms (`joint` off, or a configuration `_joint_ok` refuses) call the same two functions once per engine.  Chained
(`chain_wgrad`, their default): the two backwards run in step, block by block (backward_encoder_steps as a generator) - the bias /
LayerNorm sums of the title pass are written and those of the body pass added; every weight gradient is ONE chained problem over the
title rows and the body rows (tnr_gemm_tn_wgrad_group, accumulate = 2; `_wgrad_flush_chained`).
Every row goes through the same K order as in its own
launch: scores and losses are bit-identical to the two-launch form; parameter gradients are the same sums in another order.
With dropout on, each pass keeps its own forward-call number and sites: the two output Linears and the LayerNorm backwards behind
them take one site split at the pass boundary (tnr_gemm_nt_do_split / tnr_ln_bwd_do_split: rows N Lt onwards draw the body
pass's mask, row index counted from there), embeddings and attention run per pass anyway - every mask is the per-pass form's.
Student rows live in one table S = [B*(1+K) title rows | B body rows], the layout tnr_kd_embed_loss and
tnr_score_bwd already use in stage 2 with the body vector in the "user" slot.

Trainable set = the notebook's (cell 17): heads + transform matrices + encoder layers 2 and 3 of the frozen UniLM
(`trainable_layers`); optimiser = its plain Adam with two rates (cell 18: 1e-6 for bert_model, 1e-5 for the rest) via
step(lr, lr_bert, amsgrad=False).  The notebook trains under .train() (cell 19:6), i.e. with the UniLM config's dropout
(hidden 0.1, attention probabilities 0.1) live in the encoder: set_dropout() turns the same four sites on (counter-based masks,
csrc/dropout.h; the title and the body pass draw independent masks, as two passes through nn.Dropout do).
"""
import torch

import tnr_hip as T
from engine import Engine, EngineConfig, _ReduceBatch, _fork_join


class Stage1Engine:
    def __init__(self, n_layers=4, trainable_layers=(0, 1, 2, 3), num_teachers=4, npratio=4, title_len=30, body_len=256,
                 device="cuda:0", batch=32, dtype="fp16", **dims):
        """dims: hidden, heads, inter, news_dim, news_query, vocab, ... (EngineConfig keywords)."""
        # num_teachers = 0 is stage 0: TitleBodySimModel of Domian-specific_Post-train.ipynb (cells 10-11), plain CE
        common = dict(n_layers=n_layers, trainable_layers=trainable_layers, num_teachers=num_teachers, user_log_length=0,
                      temperature=1.0, coef=1.0, stage1=True, **dims)
        self.cfg_t = EngineConfig(npratio=npratio, num_words=title_len, **common)
        self.cfg_b = EngineConfig(npratio=0, num_words=body_len, **common)
        # the title engine's per-token / per-sequence workspaces have room for the body pass's rows / sequences behind its own (joint passes)
        self.title = Engine(self.cfg_t, device, max_batch=batch, dtype=dtype, extra_rows=batch * body_len, extra_seqs=batch)
        self.body = Engine(self.cfg_b, device, max_batch=batch, dtype=dtype, share=self.title)
        self.dev = self.title.dev
        self.ws = None               # slabs of the chained weight gradients (allocated by the first backward)

    def set_dropout(self, p_hidden, p_attn, seed):
        """Train-mode dropout of both encoder passes (tnlrv3/config/*.json:2,4 under Post-train_KD.ipynb cell 19:6)."""
        self.title.set_dropout(p_hidden, p_attn, seed, pass_id=0)
        self.body.set_dropout(p_hidden, p_attn, seed, pass_id=1)

    # parameters / optimiser state are the title engine's
    def load_state_dict(self, sd):
        self.title.load_state_dict(sd)
        self.body.refresh_rel()

    def state_dict(self):
        return self.title.state_dict()

    def ema_state_dict(self):
        """Engine.ema_state_dict of the one average over the shared parameters (step(ema_decay=...)); None if it was never on."""
        return self.title.ema_state_dict()

    def load_ema_state_dict(self, sd):
        self.title.load_ema_state_dict(sd)

    @property
    def ema_updates(self):
        return self.title.ema_updates

    def optimizer_state_dict(self):
        """Engine.optimizer_state_dict of the title engine, which owns the shared buffers, the step count and the scaler;
        "dropout_calls" is the pair [title, body]: each pass numbers its own forward calls (set_dropout)."""
        osd = self.title.optimizer_state_dict()
        osd["dropout_calls"] = [int(self.title.drop_calls), int(self.body.drop_calls)]
        return osd

    def load_optimizer_state_dict(self, osd):
        """After load_state_dict() / load_ema_state_dict(): Engine.load_optimizer_state_dict on the title engine, then both
        passes' dropout call counters."""
        calls = osd["dropout_calls"]
        if not isinstance(calls, (list, tuple)) or len(calls) != 2:
            raise ValueError("optimiser state: dropout_calls must be the pair [title, body] for a Stage1Engine, got %r" % (calls,))
        self.title.load_optimizer_state_dict(dict(osd, dropout_calls=int(calls[0])))
        self.body.drop_calls = int(calls[1])

    def grad(self, name):
        return self.title.grad(name)

    @property
    def shapes(self):
        return self.title.shapes

    def forward_indexed(self, title_table, body_table, idx, label, t_title_tables, t_body_tables, body_idx=None):
        """The same step fed by index (DistillDataset.__getitem__, cell 8, at index level): title_table (n, 2Lt) and
        body_table (n, 2Lb) int32 token tables and teacher tables (T, n, D) fp32 stay in HBM; idx (B, 1+K) int32 holds the
        positive document first, then its sampled negatives (the body is the positive's).  body_idx (B,) int32 contiguous = idx[:, 0]
        if the loader has it (saves the step its one strided copy)."""
        t = self.title
        B, T_ = idx.shape[0], self.cfg_t.T
        assert idx.shape[1] == self.cfg_t.C
        N, Rt = self._begin(B, label)
        D = self.cfg_t.D
        tidx = idx.reshape(-1).to(torch.int32).contiguous()
        bidx = idx[:, 0].to(torch.int32).contiguous() if body_idx is None else body_idx

        def teacher_side():
            # the teacher side (row gathers, teacher scores, projections) needs nothing of the student's: in front of the title pass,
            # where it runs beside the start of the body pass instead of alone between the encoders and the losses
            if T_:
                T.call("tnr_gather_rows", t_title_tables, t_title_tables.shape[1], tidx, N, D, T_, t.X, t.X.shape[1], 0)
                T.call("tnr_gather_rows", t_body_tables, t_body_tables.shape[1], bidx, B, D, T_, t.X, t.X.shape[1], N)
                self._teacher_side(B, N, Rt)
        return self._encode_heads(B, N, Rt, title_table, tidx, body_table, bidx, teacher_side)

    def forward(self, title, body, label, teacher_titles, teacher_bodies):
        """title (B,1+K,2Lt) / body (B,2Lb) int64 [ids | mask]; label (B,); teacher_* lists of (B,1+K,D) / (B,D) fp32
        (or stacked (T,B,1+K,D) / (T,B,D)).  -> (losses [distill, target, emb, -], score (B,1+K))."""
        t, b = self.title, self.body
        cfg = self.cfg_t
        B = title.shape[0]
        C, D, T_ = cfg.C, cfg.D, cfg.T
        assert title.shape[1:] == (C, 2 * cfg.L) and body.shape == (B, 2 * self.cfg_b.L)
        N, Rt = self._begin(B, label)
        b.tok[:B].copy_(body)
        t.tok[:N].copy_(title.reshape(N, 2 * cfg.L))
        for i in range(T_):
            t.X[i, :N].copy_(teacher_titles[i].reshape(N, D))
            t.X[i, N:Rt].copy_(teacher_bodies[i].reshape(B, D))

        def teacher_side():
            if T_:
                self._teacher_side(B, N, Rt)
        return self._encode_heads(B, N, Rt, t.tok[:N], None, b.tok[:B], None, teacher_side)

    def _begin(self, B, label):
        """Workspaces for a batch of B, the form this step takes (ran_joint) and its label -> (title sequences, student rows)."""
        self._prepare(B)
        self.ran_joint = self._joint_ok()      # (before anything is copied into the workspaces: it may lay them out afresh)
        N = B * self.cfg_t.C
        self.cur = (B, N, N + B)
        self.title.label = label.to(torch.int64).contiguous()
        return N, N + B

    def _parts(self, B, N):
        """The joint passes as parts of the title engine's buffers (engine.py, _per_part): the bodies' rows behind the titles'."""
        return [(self.title, N, 0, 0), (self.body, B, N * self.cfg_t.L, N)]

    def _stream_if(self, on):
        return self._side_stream() if (on and self.dev.type == "cuda") else None

    def _encode_heads(self, B, N, Rt, title_tok, tidx, body_tok, bidx, teacher_side):
        """Both encoder passes (the bodies first: cell 12), news vectors -> S[:N] (titles), S[N:N + B] (bodies); then the heads."""
        t, b = self.title, self.body
        if self.ran_joint:
            t.encode(title_tok, N, nidx=tidx, parts=self._parts(B, N), src2=(body_tok, bidx), side=self._stream_if(self.joint_streams),
                     before=teacher_side)
        else:
            def title_pass():
                teacher_side()
                t.encode(title_tok, N, nidx=tidx)
            _fork_join(self._stream_if(self.two_streams), lambda: b.encode(body_tok, B, nidx=bidx, out=t.S[N:]), title_pass)
        return self._heads(B, N, Rt)

    # The body pass on a second stream beside the title pass: most launches of either pass are partial rounds (4 800 / 4 096 token
    # rows at 30 / 128: 228 / 192 tiles for 256 CUs), side by side they fill the chip.  The same kernels on the same operands:
    # bit-identical to one stream (test_stage1_chained_weight_gradients_equal_the_two_pass_form); 2.46 -> 2.14 ms per step.
    two_streams = True

    def _prepare(self, B):
        t, b = self.title, self.body
        if B != t.B_alloc:                       # a short last batch: the body rows sit directly behind THIS batch's title rows
            t.extra_rows, t.extra_seqs = B * self.cfg_b.L, B
        t._prepare(B)
        b._prepare(B)

    # ------------------------------------------------------------------ joint passes (round 6)
    joint = True            # False: one launch per pass for everything (the round-5 form; tools/ A/B, tests)
    joint_streams = False   # True: the body's per-pass kernels (embeddings, attention, pooling) on the second stream beside the title's.
                            # Measured (interleaved legs, one box): 1.816 -> 1.718 ms at 30 / 128 and 3.830 -> 3.717 at 24 / 512 WITHOUT it -
                            # ten fork / join pairs per step cost more than running two short kernels side by side wins
    joint_group_wgrad = True    # the joint passes' weight gradients of a layer in ONE persistent launch + one slab sum
    _side = None            # _side_stream(): the second stream (two_streams, joint_streams), made when first asked for
    _joint_rows_written = False     # _joint_ok(): the last step laid body rows behind the title engine's own

    def _joint_ok(self):
        t, b = self.title, self.body
        cfg = self.cfg_t
        same = lambda d: None if d is None else (d["p_hidden"], d["p_attn"], d["seed"])
        ok = bool(self.joint and same(t.drop) == same(b.drop) and cfg.pooling == "att" and self.dev.type == "cuda"
                  and t.fcache is None and t.group_wgrad is False
                  # the grouped weight gradients that share one round (Engine._wgrad_flush) take 256 x 256 tiles only (an
                  # inter = 128 * odd config runs per pass instead)
                  and (not self.joint_group_wgrad or (cfg.H % 256 == 0 and cfg.I % 256 == 0)))
        if not ok and self._joint_rows_written:
            # a per-pass step after joint ones (a tools/ A/B, `joint` switched off): the title engine's own kernels rely on ZERO rows
            # behind its N Lt rows (the weight gradient reads up to the next multiple of 64), where the joint passes have put body
            # rows - lay the title workspace out afresh, once.  The body engine's recorded reduction tables go with it: its backward
            # reads its rows of dvec from the TITLE engine's dS (backward: dS[N:Rt]), so a table recorded by an earlier per-pass step
            # carries the address of the buffer that was just replaced
            t._alloc_workspace(t.B_alloc)
            b.red.clear()
        self._joint_rows_written = ok
        return ok

    def _side_stream(self):
        if self._side is None:
            self._side = torch.cuda.Stream(self.dev)
        return self._side

    def _teacher_side(self, B, N, Rt):
        """Teacher scores <title_emb[b, c], body_emb[b]> and the teachers' projections from the teacher rows X: independent fp32
        GEMMs of a few microseconds each - one grouped launch (each computed exactly as by its own tnr_sgemm call)."""
        t = self.title
        C, D, T_ = self.cfg_t.C, self.cfg_t.D, self.cfg_t.T
        X = t.X
        group = [t._sgemm_problem(X[i], D, 1, C * D, X[i, N:], D, 1, D, t.t_score[i], 1, C, None, 0, C, 1, D, batch=B) for i in range(T_)]
        Wt = t._view("transform_matrix.0.weight", T_ * D * D, (T_, D, D))
        bt = t._view("transform_matrix.0.bias", T_ * D, (T_, D))
        group.append(t._sgemm_problem(X, D, 1, X.stride(0), Wt, D, 1, D * D, t.Pm, D, t.Pm.stride(0), bt, D, Rt, D, D, batch=T_))
        for i in range(0, len(group), 8):
            t._sgemm_group(group[i:i + 8])

    def _heads(self, B, N, Rt):
        """Scores, teacher weights and the three losses from the student rows S and the teacher rows X."""
        t = self.title
        cfg = self.cfg_t
        C, D, T_ = cfg.C, cfg.D, cfg.T
        S = t.S[:Rt]
        # score[b, c] = <title_vec[b, c], body_vec[b]>
        t._sgemm(S, D, 1, C * D, S[N:], D, 1, D, t.score, 1, C, None, 0, C, 1, D, batch=B)
        T.call("tnr_kd_score_loss", t.score, t.t_score if T_ else None, t.label, 1.0, 1.0, t.tw if T_ else None, t.dscore,
               t.losses, B, C, T_)
        if T_:
            T.call("tnr_kd_embed_loss", S, t.Pm, t.tw, t.losses[2:], t.dS, t.dP, t.kd_part, B, 0, C, D, T_)
        else:
            t.dS[:Rt].zero_()
            t.losses[2:3].zero_()
        return t.losses, t.score[:B]

    @torch.no_grad()
    def encode_table(self, table, which):
        """Embeddings of every row of a resident token table (Domian-specific_Post-train.ipynb cells 20-22: the teacher
        title / body embeddings stage 1 distils from).  which: "title" | "body".  -> (n, D) fp32 on device."""
        eng = self.title if which == "title" else self.body
        assert table.shape[1] == 2 * eng.cfg.L
        return eng.encode_news(table)

    def total_loss(self):
        """target + distill + emb (cell 14) as a device scalar."""
        l = self.title.losses
        return l[0] + l[1] + l[2]

    def backward(self, after_bucket=None):
        """Gradients of total_loss -> the shared flat_g.  Buckets complete (and after_bucket fires) during the body
        pass, the second and accumulating one."""
        t, b = self.title, self.body
        t._red_check()
        b._red_check()
        B, N, Rt = self.cur
        C, D = self.cfg_t.C, self.cfg_t.D
        S, dS = t.S[:Rt], t.dS
        # the heads batch of the backward that follows (backward_encoder_steps' key): over both parts' sequences, or the title pass's -
        # merged into one reduction at its end unless it flushes by bucket (under a hook the chained title pass gets one of its own)
        if self.ran_joint:
            key = ("heads", "joint", N + B, after_bucket is None and t.merge_reductions)
        else:
            key = ("heads", 0, N, t.merge_reductions and not (self.chain_wgrad and after_bucket is not None))
        pend = []                 # the transform matrices' gradient GEMM rides in the title pass's first grouped launch
        if self.cfg_t.T:
            t._transform_grads(Rt, t.red.setdefault(key, _ReduceBatch(t.dev)), pend)
        T.call("tnr_score_bwd", S, t.cidx, S[N:], t.dscore, dS, dS[N:], B, C, D)
        if self.ran_joint:
            # always writes; a layer's weight gradients leave in one grouped launch whose units share one round (Engine._wgrad_flush)
            t.backward_encoder(dS[:Rt], N, after_bucket=after_bucket, pend=pend, parts=self._parts(B, N),
                               side=self._stream_if(self.joint_streams), group_wgrad=self.joint_group_wgrad)
            return
        if not self.chain_wgrad:
            t.backward_encoder(dS[:N], N, acc=0, pend=pend)
            b.backward_encoder(dS[N:Rt], B, acc=1, after_bucket=after_bucket)
            return
        # The two passes' backwards in step, layer by layer: every shared weight gets ONE chained weight-gradient problem (title
        # rows, then body rows; one fixed-order slab sum) instead of a launch + slab sum that writes and a launch + slab sum that
        # adds.  The title's segment runs first, so wherever both flush partial sums the writing flush precedes the adding one;
        # under a bucket hook the title pass flushes bucket by bucket as well (a hook of its own that does nothing).
        hooked = after_bucket is not None
        gt = t.backward_encoder_steps(dS[:N], N, acc=0, after_bucket=(lambda i: None) if hooked else None, defer=True, split_ffn=hooked,
                                      pend=pend)
        gb = b.backward_encoder_steps(dS[N:Rt], B, acc=1, after_bucket=after_bucket, defer=True, split_ffn=hooked)
        # side by side only when BOTH passes hold their partial sums back for one merged reduction at the very end: with
        # Engine.merge_reductions off (tools/step_ab.py) each pass flushes inside its own segments, and the title's writing flush
        # (main stream) would be unordered against the body's adding flush (side stream) on the shared bias / LayerNorm gradients
        if not (self.two_streams and not hooked and self.dev.type == "cuda" and t.merge_reductions and b.merge_reductions):
            while True:
                at, ab = next(gt, None), next(gb, None)
                assert at == ab, (at, ab)
                if at is None:
                    break
                self._wgrad_flush_chained()
            return
        # ... and side by side: the body pass's segments on the second stream.  What the two passes share are the gradients: the
        # weights' are written by the chained launches (main stream, both passes joined in front of it, released behind it); all
        # others go through the two passes' batched reductions, which without a bucket hook run once, at the very end - the
        # title's (writing) and then the body's (adding), both on the main stream behind the join; the one gradient written
        # directly - dense.weight, first thing in the heads segment - orders the body's heads segment behind the title's.
        main, side = torch.cuda.current_stream(self.dev), self._side_stream()
        side.wait_stream(main)
        first = True
        while True:
            at = next(gt, None)
            if at is None:                      # the title's merged reduction has been launched: the body's follows on the same stream
                main.wait_stream(side)
                assert next(gb, None) is None
                break
            if first:
                side.wait_stream(main)
                first = False
            with torch.cuda.stream(side):
                ab = next(gb, None)
            assert at == ab, (at, ab)
            main.wait_stream(side)
            self._wgrad_flush_chained()
            side.wait_stream(main)

    chain_wgrad = True      # False: the title pass writes, the body pass accumulates (two launches + two slab sums per weight)

    def _wgrad_flush_chained(self):
        t, b = self.title, self.body
        pt, pb = t._wg_defer, b._wg_defer
        assert len(pt) == len(pb) and t.ginv == b.ginv
        if self.ws is None or self.ws.numel() < 2 * t.ws.numel():
            self.ws = torch.zeros(2 * t.ws.numel() + 256, device=self.dev, dtype=torch.float32)
        probs, off = [], 0
        for (dy1, x1, dw, M1, N_, K_, acc1), (dy2, x2, dw2, M2, N2, K2, acc2) in zip(pt, pb):
            assert dw.data_ptr() == dw2.data_ptr() and (N_, K_) == (N2, K2) and acc1 == 0 and acc2 == 1
            total = t._wgrad_splits(N_, K_)[0]                   # the units of one round, shared out by rows
            s1 = min(max(1, round(total * M1 / (M1 + M2))), max(1, total - 1))
            s2 = max(1, total - s1)
            elems = (s1 + s2) * N_ * K_
            common = dict(dW=dw, lddw=dw.stride(0), N=N_, K=K_, out_scale=t.ginv)
            probs.append(dict(common, dY=dy1, lddy=dy1.stride(0), X=x1, ldx=x1.stride(0), M=M1, ws=self.ws[off:off + elems], splits=s1,
                              accumulate=0))
            probs.append(dict(common, dY=dy2, lddy=dy2.stride(0), X=x2, ldx=x2.stride(0), M=M2, ws=None, splits=s2, accumulate=2))
            off += (elems + 63) // 64 * 64
            assert off <= self.ws.numel()
        for i in range(0, len(probs), 4):
            T.wgrad_group(probs[i:i + 4], f16=t.f16)
        del pt[:], pb[:]

    def bucket_ranges(self):
        return self.title.bucket_ranges()

    def step(self, lr, grad_scale=1.0, lr_bert=None, amsgrad=False, **kw):
        """Post-train_KD.ipynb cell 18: optim.Adam([{bert_model, 1e-6}, {rest, 1e-5}]) (plain Adam by default here).
        kw: Engine.step's sync, max_grad_norm, weight_decay, warmup_steps, lr_decay_steps, ema_decay, ema_warmup, lamb (one decay map,
        one schedule position, one average, one chunk table: the title engine owns the shared buffers)."""
        self.title.step(lr, grad_scale, lr_bert=lr_bert, amsgrad=amsgrad, **kw)

    @property
    def lr_scale(self):
        """Engine.lr_scale of the last step(warmup_steps=, lr_decay_steps=): the host's schedule multiplier, None without one."""
        return self.title.lr_scale

    def grad_norm(self):
        """Engine.grad_norm of the last step(max_grad_norm=...): one norm over the title + body gradient (one flat buffer)."""
        return self.title.grad_norm()

    def trust_ratios(self):
        """Engine.trust_ratios of the last step(lamb=True): one chunk table over the shared flat buffer."""
        return self.title.trust_ratios()
