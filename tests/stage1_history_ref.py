"""Shared by tests/test_stage1_history_ref_cpu.py and tests/test_stage1_history_gpu.py: one small stage-1 model, resident title and
body tables, five step feeds and the SCHEDULES of unlike steps that one long-lived Stage1Engine is driven through.  Modelled on
tests/history_ref.py; imports no GPU module.

Stage 1 carries more from one step to the next than stage 2 ("state that crosses steps"): the body pass's rows lie
directly behind the title pass's inside the title engine's buffers, so the boundary moves with the batch (Stage1Engine._prepare);
a per-pass step behind joint ones has the title workspace laid out afresh, once (_joint_ok / _joint_rows_written); the chained
weight gradients have slabs of their own; two engines share a scaler and parameters but neither workspaces nor reduction tables;
the dropout buffers are sized from the workspace.  The schedules visit the step pairs at which each of them could go wrong; the
GPU test compares every step, bit for bit, with the same step on a fresh engine.

Model: hidden 256, 4 heads, inter 512 (H % 256 == 0 and I % 256 == 0: _joint_ok can say yes), two layers, both trainable, two
teachers, news_dim 64, query 72, vocab 2000, 128 positions; 1 + 3 titles of Lt = 17 (the L <= 32 attention kernels), bodies of
Lb = 72 (> AP_LONG = 64: the chunked pooling kernels with an 8-token last chunk, the long attention kernels at Lr = 96).
  batch   title rows       body rows        joint rows       the body part starts at
  full 6  408 (% 64 = 24)  432 (% 64 = 48)  840 (% 64 = 8)   408 (% 32 = 24)
  short 4 272 (% 64 = 16)  288 (% 64 = 32)  560 (% 64 = 48)  272 (% 32 = 16)
Every pass and both joint layouts have a tail inside their last 64-row tile; the body part never starts on a multiple of 32.

A feed is (idx (B, 1 + K) int32 rows of the tables, positive first; label (B,) int64).  A schedule is a list of step records
(step()): feed id, feed form ("idx": resident tables + indices, "idx_body": the same with body_idx given, "tok": token rows and
teacher vectors themselves), the engine's switches (joint, two_streams, joint_streams, chain_wgrad), bucket hook, dropout
(p_hidden, p_attn, seed) or None, the fp16 scaler multiplier, `only` (a 16-bit type the step is for) and `pre`: actions on the
engine in front of the step - ("encode_table", "title" | "body"), ("step", lr)."""
import numpy as np

import hashinit
import synth
from schema import FULL, state_shapes
from oracle import newsrec_oracle as O

H, A, I, NL, TR, D, Q, T_, VOCAB, MAX_POS = 256, 4, 512, 2, (0, 1), 64, 72, 2, 2000, 128
K, LT, LB = 3, 17, 72
C = 1 + K
B_FULL, B_SHORT = 6, 4
N_DOCS = 300                                   # + the pad row 0: 301 rows, no multiple of 24, 16, 6 or 4 (encode_table's pass sizes)
AP_LONG = 64                                   # engine.AP_LONG (asserted by the GPU file): longer sequences take the chunked pooling
LR = 1e-3                                      # schedule C: Adam moves every element by about lr, 8 bf16 ulps of a 0.03 weight
FEEDS = {"full_a": B_FULL, "full_b": B_FULL, "full_c": B_FULL, "short_a": B_SHORT, "short_b": B_SHORT}
FORMS = ("idx", "idx_body", "tok")


def dims():
    return dict(FULL, H=H, A=A, I=I, Q=Q, vocab=VOCAB, max_pos=MAX_POS)


def oracle_cfg():
    return dict(n_layers=NL, heads=A, trainable_layers=list(TR))


def engine_kwargs():
    """Keyword arguments of Stage1Engine for the model (without device, batch and dtype)."""
    return dict(n_layers=NL, trainable_layers=TR, num_teachers=T_, npratio=K, title_len=LT, body_len=LB, hidden=H, heads=A, inter=I,
                news_dim=D, news_query=Q, vocab=VOCAB, max_pos=MAX_POS)


def rows(B):
    """-> (title rows, body rows, joint rows) of a batch; the body part of a joint pass starts at the first."""
    return B * C * LT, B * LB, B * C * LT + B * LB


_MEMO = {}


def _once(key, make):
    if key not in _MEMO:
        _MEMO[key] = make()
    return _MEMO[key]


def weights():
    """Hash-initialised state dict (numpy), built once and never modified."""
    return _once("P", lambda: hashinit.init_state_dict(93, state_shapes(dims(), NL, D, T_)))


def table(which):
    """The resident token table of the titles (301, 2 Lt) or the bodies (301, 2 Lb), int32 [ids | mask], row 0 all zero."""
    make = {"title": lambda: synth.news_table(21, N_DOCS, LT, vocab=VOCAB),
            "body": lambda: synth.news_table(22, N_DOCS, LB, vocab=VOCAB, mean_len=52.0, std_len=14.0)}[which]
    return _once(("table", which), make)


def teachers(which):
    """The teachers' title / body tables (T, 301, D) float32."""
    seed = {"title": 23, "body": 24}[which]
    return _once(("teachers", which), lambda: synth.teacher_tables(seed, T_, N_DOCS, D).astype(np.float32))


def _draw(fid):
    B = FEEDS[fid]
    rs = np.random.RandomState(2000 + sorted(FEEDS).index(fid))
    idx = 1 + rs.permutation(N_DOCS)[:B * C].reshape(B, C)            # distinct documents, rows in [1, 300]
    return idx.astype(np.int32), rs.randint(0, C, B).astype(np.int64)


def feed(fid):
    """-> (idx (B, 1 + K) int32, label (B,) int64), built once."""
    return _once(("feed", fid), lambda: _draw(fid))


def tokens(fid):
    """The feed at token level, gathered from the same tables: (title (B, 1 + K, 2 Lt) int64, body (B, 2 Lb) int64, label,
    [teacher title vectors (B, 1 + K, D)] x T, [teacher body vectors (B, D)] x T) - what Stage1Engine.forward and O.distill_fwd take."""
    def make():
        idx, y = feed(fid)
        tt, tb = teachers("title"), teachers("body")
        return (table("title").astype(np.int64)[idx], table("body").astype(np.int64)[idx[:, 0]], y,
                [tt[i][idx] for i in range(T_)], [tb[i][idx[:, 0]] for i in range(T_)])
    return _once(("tok", fid), make)


# ---------------------------------------------------------------------------------------------------------------- schedules
def step(fid, form="idx", joint=True, hook=False, two_streams=True, joint_streams=False, chain_wgrad=True, drop=None, mult=1.0,
         only=None, pre=(), anchor=False):
    assert fid in FEEDS and form in FORMS
    return dict(feed=fid, B=FEEDS[fid], form=form, joint=joint, hook=hook, two_streams=two_streams, joint_streams=joint_streams,
                chain_wgrad=chain_wgrad, drop=drop, mult=mult, only=only, pre=tuple(pre), anchor=anchor)


BOTH = [("encode_table", "title"), ("encode_table", "body")]
# A: fixed weights, no dropout
SCHEDULE_A = [
    step("full_a"),                                                        # joint: 840 rows, the bodies from row 408
    step("full_b", hook=True),                                             # joint, bucket by bucket
    step("full_c", joint=False),                                           # per pass behind joint steps: the title workspace re-laid
    step("full_a", joint=False, hook=True),                                # the chained, hooked form
    step("full_b"),                                                        # joint again (no re-lay on the way back)
    step("short_a", form="tok", anchor=True),                              # SHORT: the boundary moves from row 408 to row 272
    step("short_b", joint=False),
    step("short_a", hook=True),
    step("full_c", form="tok"),                                            # and back
    step("full_a", joint=False, two_streams=False, pre=BOTH),              # eval passes through the same per-token buffers
    step("full_b", joint_streams=True, pre=BOTH),
    step("full_c", joint=False, chain_wgrad=False),                        # the writing / adding form behind chained steps
    step("full_a", form="idx_body", joint=False),                          # chained again: records the key the scale steps replay
    step("full_a", joint=False, mult=0.5, only="fp16"),                    # the loss scale moves under a recorded key ...
    step("full_a", joint=False, mult=1.0, only="fp16"),                    # ... and back
    step("full_a"),                                                        # the first step again
    step("full_a", mult=0.5, only="fp16"),                                 # the same in the joint form
    step("full_a", mult=1.0, only="fp16"),                                 # (fp16: the first step's bits once more)
]

DROP = (0.1, 0.1, 4242)
# B: dropout toggled on one engine
SCHEDULE_B = [
    step("full_a"),
    step("full_a", drop=DROP),
    step("short_a", drop=DROP),                                            # dyprem / dh1prem re-made with the workspace
    step("short_b", joint=False, drop=DROP),                               # ... and again by the re-lay of the title workspace
    step("full_b", drop=DROP, pre=BOTH),                                   # train=False passes: no call number, no mask
    step("full_a"),
]

# C: the weights move between unlike steps
SCHEDULE_C = [
    step("full_a"),
    step("short_a", joint=False, pre=[("step", LR)]),
    step("full_b", hook=True, pre=[("step", LR)]),
    step("full_c", pre=[("step", LR)]),
]
SCHEDULES = dict(A=SCHEDULE_A, B=SCHEDULE_B, C=SCHEDULE_C)


def steps_for(schedule, dtype):
    """The schedule's records for a 16-bit type (the fp16-only filter)."""
    return [r for r in schedule if r["only"] in (None, dtype)]


def key_form(rec):
    """What tells the recorded reduction tables of the step apart (stage1.py, Stage1Engine.backward; engine.py,
    backward_encoder_steps): the batch, the form, whether all partial sums leave in one batch (no bucket hook), and for the
    per-pass form whether the weight gradients are chained."""
    return rec["B"], rec["joint"], not rec["hook"], (rec["joint"] or rec["chain_wgrad"])


def epochs(recs):
    """Per record, the number of the workspace it runs in: a new one when the batch changes (_prepare) and when a per-pass step
    follows a joint one (_joint_ok lays the title workspace out afresh; the recorded tables die with it)."""
    out, e = [], 0
    for i, r in enumerate(recs):
        if i and (r["B"] != recs[i - 1]["B"] or (recs[i - 1]["joint"] and not r["joint"])):
            e += 1
        out.append(e)
    return out


def anchor_oracle():
    """-> (oracle output of O.distill_fwd, {key: gradient} of O.distill_bwd) for schedule A's anchor step, computed once."""
    def make():
        rec, = [r for r in SCHEDULE_A if r["anchor"]]
        out = O.distill_fwd(weights(), oracle_cfg(), *tokens(rec["feed"]))
        return out, O.distill_bwd(weights(), oracle_cfg(), out)
    return _once("anchor", make)
