"""Shared by tests/test_history_ref_cpu.py and tests/test_step_history_gpu.py: one small model, a resident news table, a dozen
step feeds and the SCHEDULES of unlike steps that one long-lived Engine is driven through.  Imports no GPU module.

Every other engine test builds a fresh Engine per step shape; a run keeps one engine for all of them.  What an engine carries from
one step to the next ("state that crosses steps") is valid only by construction: zero rows behind the token rows that the
weight-gradient kernels read, recorded reduction tables, caches, lazily made buffers, scratch shared with the forward-only paths.
The schedules visit the step pairs at which each of them could go wrong; the GPU test compares every step, bit for bit, with the
same step on a fresh engine.

Model: hidden 256, 4 heads, inter 512, two layers of which layer 1 trains (layer 0 frozen: build_frozen_cache applies), attention
pooling, two teachers, news_dim 64, query 72, vocab 2000, user_log_mask off; U, C, L = 20, 5, 17.
  full batch  B = 6: 150 slots, 2 550 token rows (2 550 % 64 = 54);  short batch B = 4: 100 slots, 1 700 rows (1 700 % 64 = 36):
  both have a tail behind their rows inside the last 64-row tile.  Plans (quantum 64) encode 64 x 17 = 1 088 or 128 x 17 = 2 176
  rows, multiples of 64: a plan that shrinks has the previous step's live rows directly behind its own.

A feed is (hist_idx, mask, cand_idx, label) drawn from a RandomState over a pool sized for the distinct count it is here for
(synth.impressions' skew gives 24 - 73 distinct news at these shapes and never a None plan): <= 64 distinct -> n_enc 64,
65 - 128 -> 128, more than 128 at B = 6 -> build_plan returns None.  Row 1 of every history is fully masked, the first slots of
every history are the padding news 0.

A schedule is a list of step records (step()): feed id, plan yes / no, feed form ("idx": resident tables + indices, "tok": the
token rows and teacher vectors themselves), bucket hook, micro (j, K), dropout (p_hidden, p_attn, seed) or None, the fp16 scaler
multiplier, `only` (a 16-bit type the step is for) and `pre`: actions on the engine in front of the step."""
import numpy as np

import hashinit
import synth
from dedup import build_plan
from schema import FULL, state_shapes
from oracle import newsrec_oracle as O

BERT = O.BERT
H, A, I, NL, TR, D, Q, T_, VOCAB, MAX_POS = 256, 4, 512, 2, (1,), 64, 72, 2, 2000, 128
U, C, L = 20, 5, 17
B_FULL, B_SHORT = 6, 4
N_NEWS = 400                                   # + the pad row 0: 401 rows, no multiple of 150 or 100 (encode_news' pass size)
POOL = {64: 48, 128: 110, "q16": 40}           # ids a feed draws from, by the n_enc it is here for
LR = 1e-3                                      # schedule C: Adam moves every element by about lr, 8 bf16 ulps of a 0.03 weight

# feed id -> (batch, target): None = as many distinct news as slots (no plan), 64 / 128 = the n_enc of its plan, "q16" = at most
# 41 distinct: 48 sequences under quantum 16, 48 x 17 = 816 token rows, 816 % 64 = 48
FEEDS = {"full_a": (B_FULL, None), "full_b": (B_FULL, None), "full_c": (B_FULL, None),
         "p128_a": (B_FULL, 128), "p128_b": (B_FULL, 128), "p128_c": (B_FULL, 128),
         "p64_a": (B_FULL, 64), "p64_b": (B_FULL, 64), "p64_c": (B_FULL, 64),
         "short_a": (B_SHORT, None), "short_b": (B_SHORT, None), "short_p64": (B_SHORT, 64),
         "q16": (B_FULL, "q16")}


def dims():
    return dict(FULL, H=H, A=A, I=I, Q=Q, vocab=VOCAB, max_pos=MAX_POS)


def oracle_cfg():
    return dict(n_layers=NL, heads=A, trainable_layers=list(TR), user_log_mask=False, temperature=1.5, coef=0.3, pooling="att",
                nrms_heads=0)


def engine_kwargs():
    """Keyword arguments of EngineConfig for the model."""
    return dict(n_layers=NL, trainable_layers=TR, hidden=H, heads=A, inter=I, num_teachers=T_, user_log_length=U, npratio=C - 1,
                num_words=L, news_dim=D, news_query=Q, user_query=Q, user_log_mask=False, temperature=1.5, coef=0.3, pooling="att",
                nrms_heads=0, vocab=VOCAB, max_pos=MAX_POS)


def rows(B):
    """Token rows of an un-deduplicated pass."""
    return B * (U + C) * L


_MEMO = {}


def _once(key, make):
    if key not in _MEMO:
        _MEMO[key] = make()
    return _MEMO[key]


def weights():
    """Hash-initialised state dict (numpy), built once and never modified."""
    return _once("P", lambda: hashinit.init_state_dict(91, state_shapes(dims(), NL, D, T_, "att", 0)))


def news():
    """The resident token table (401, 2 L) int32 [ids | mask], row 0 the all-zero pad news."""
    return _once("news", lambda: synth.news_table(5, N_NEWS, L, vocab=VOCAB))


def teachers():
    """The teachers' tables (T, 401, D) float32."""
    return _once("teachers", lambda: synth.teacher_tables(5, T_, N_NEWS, D).astype(np.float32))


def _draw(fid):
    B, target = FEEDS[fid]
    rs = np.random.RandomState(1000 + sorted(FEEDS).index(fid))
    n = B * (U + C)
    if target is None:
        ids = 1 + rs.permutation(N_NEWS)[:n]
    else:
        pool = 1 + rs.permutation(N_NEWS)[:POOL[target]]
        ids = pool[rs.randint(0, pool.size, n)]
    h, c = ids[:B * U].reshape(B, U).copy(), ids[B * U:].reshape(B, C).copy()
    m = (rs.rand(B, U) > 0.25).astype(np.float32)
    m[1] = 0                                           # a history with nothing in it
    for b in range(B):                                 # left padding with the pad news, as the loader lays a short history out
        k = 2 if b == 0 else rs.randint(0, 4)
        h[b, :k], m[b, :k] = 0, 0
    return h.astype(np.int32), m, c.astype(np.int32), rs.randint(0, C, B).astype(np.int64)


def feed(fid):
    """-> (hist_idx (B, U) int32, mask (B, U) float32, cand_idx (B, C) int32, label (B,) int64), built once."""
    return _once(("feed", fid), lambda: _draw(fid))


def plan(fid, quantum=64):
    """build_plan of the feed (numpy members), or None."""
    h, _, c, _ = feed(fid)
    return _once(("plan", fid, quantum), lambda: build_plan(h, c, quantum=quantum))


def tokens(fid):
    """The feed at token level, gathered from the same tables: (hist (B, U, 2L) int64, mask, cand (B, C, 2L) int64, label,
    [teacher history vectors (B, U, D)] x T, [teacher candidate vectors (B, C, D)] x T) - what Engine.forward and O.model_fwd take."""
    def make():
        h, m, c, y = feed(fid)
        comb, tt = news().astype(np.int64), teachers()
        return comb[h], m, comb[c], y, [tt[i][h] for i in range(T_)], [tt[i][c] for i in range(T_)]
    return _once(("tok", fid), make)


def named_tokens(rec):
    """Word ids (without the padding id 0) of the rows a step encodes: of its distinct news under a plan, else of every slot."""
    h, _, c, _ = feed(rec["feed"])
    ids = plan(rec["feed"]).uniq if rec["plan"] else np.concatenate([h.reshape(-1), c.reshape(-1)])
    return np.setdiff1d(np.unique(news()[ids, :L]), [0])


# ---------------------------------------------------------------------------------------------------------------- schedules
def step(fid, plan=False, form="idx", hook=False, micro=None, drop=None, mult=1.0, only=None, pre=(), anchor=False):
    assert fid in FEEDS and form in ("idx", "tok")
    return dict(feed=fid, B=FEEDS[fid][0], plan=plan, form=form, hook=hook, micro=micro, drop=drop, mult=mult, only=only,
                pre=tuple(pre), anchor=anchor)


# A: fixed weights, no optimiser step
SCHEDULE_A = [
    step("full_a"),                                                        # 2 550 rows: a tail of 10 rows inside the last tile
    step("p128_a", plan=True),
    step("p64_a", plan=True),                                              # the rows of the step before lie behind it
    step("p128_b", plan=True, pre=[("encode_news",), ("user_vectors", "full_b")]),    # other news under a recorded key
    step("p64_b", plan=True),
    step("full_b", hook=True),
    step("full_a"),                                                        # the first step again, six steps later
    step("short_a", form="tok", anchor=True),                              # the workspace is laid out anew; the eighth step
    step("short_p64", plan=True),
    step("short_b"),
    step("full_c", form="tok"),                                            # and back
    step("p64_c", plan=True, pre=[("build_frozen_cache",)]),
    step("full_b", hook=True),                                             # through the cache
    step("p128_c", plan=True, micro=(0, 2)),
    step("p64_a", plan=True, micro=(1, 2)),
    step("full_a", hook=True),                                             # the per-bucket tables of this workspace, replayed
    step("full_a", mult=0.5, only="fp16"),                                 # the loss scale moves under a recorded key ...
    step("full_a", mult=1.0, only="fp16"),                                 # ... and back
]

DROP = (0.1, 0.1, 4242)
# B: dropout toggled on one engine
SCHEDULE_B = [
    step("full_a"),
    step("full_a", drop=DROP),
    step("short_a", drop=DROP),
    step("p128_a", plan=True, drop=DROP, pre=[("encode_news_eval",)]),     # a train=False pass: no call number, no mask
    step("full_b", drop=DROP),
    step("full_a"),
]

# C: the weights move between unlike steps
SCHEDULE_C = [
    step("p128_a", plan=True, pre=[("build_frozen_cache",)]),
    step("short_a", pre=[("step", LR)]),
    step("full_a", pre=[("step", LR)]),
    step("p64_a", plan=True, pre=[("step", LR)]),
]
SCHEDULES = dict(A=SCHEDULE_A, B=SCHEDULE_B, C=SCHEDULE_C)


def n_enc(rec):
    """Sequences the step's encoder pass runs: the plan's, or every slot."""
    return plan(rec["feed"]).n_enc if rec["plan"] else rec["B"] * (U + C)


def key_form(rec):
    """What tells the recorded reduction tables of the step apart (engine.py: ("heads", form, Ns, one), (l, form, Ns, block)):
    (sequences of the pass, all partial sums in one batch = no bucket hook).  Every step here writes (form 0).  A micro-batch
    in front of the last one of its window runs without the hook."""
    hook = rec["hook"] and (rec["micro"] is None or rec["micro"][0] == rec["micro"][1] - 1)
    return n_enc(rec), not hook


def windows(schedule, dtype):
    """The schedule's steps for a 16-bit type, accumulation windows kept together: a list of lists of records."""
    recs = [r for r in schedule if r["only"] in (None, dtype)]
    out, i = [], 0
    while i < len(recs):
        k = recs[i]["micro"][1] if recs[i]["micro"] else 1
        out.append(recs[i:i + k])
        i += k
    return out


def anchor_oracle():
    """-> (losses [distill, target, emb], student scores, {key: gradient}) of the numpy oracle for schedule A's anchor step."""
    def make():
        rec, = [r for r in SCHEDULE_A if r["anchor"]]
        out = O.model_fwd(weights(), oracle_cfg(), *tokens(rec["feed"]))
        G = O.model_bwd(weights(), oracle_cfg(), out)
        return np.array([out["distill_loss"], out["target_loss"], out["emb_loss"]], np.float64), out["student_score"], G
    return _once("anchor", make)
