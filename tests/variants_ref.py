"""Shared by tests/test_variants_ref_cpu.py and tests/test_variants_gpu.py: the model, feeds, plans and schedules of
tests/history_ref.py under the news-encoder poolings and user encoders that file does not visit.  Imports no GPU module.

  name           pooling   nrms_heads        user_log_mask
  att            att       0                 False            the control: history_ref's model, with the weights below
  mean_ulm       mean      0                 True
  cls_nrms       cls       4 (4 x 16 = D)    False
  att_nrms_ulm   att       4                 True
  cls_add        cls       0                 False            trainable embeddings only (with mean_ulm): what the torch port can follow

Weights: hashinit.init_state_dict(91, ...) over the variant's keys, with every `.weight` of the student's user encoder and the news
encoder's dense.weight multiplied by BOOST[variant]: 4, and 2 for cls_nrms.  With the plain hash weights the NRMS outputs are nearly
identical rows and the user pooling head behind them has oracle gradient norms of 5e-12 .. 2e-10 against a largest norm of 0.61
(att_nrms_ulm, feed short_a); mean_ulm's user_encoder.attn.att_fc1.bias sits at 8.6e-7 of 0.50: a relative comparison there would
test noise.  A factor of 6 (cls_nrms) or 8 overflows the oracle's NRMS softmax, which like the reference takes exp() without
subtracting the maximum.  cls_nrms takes 2: at 4 some queries' sums of exp() come down to the 1e-8 the reference adds to the
denominator, the attention rows stop summing to one and W_K.bias stops being a no-op - the oracle's own gradient there is 2.1e-2
(1.1e-2 on the plan feed; 4.4e-6 at 3, 7.0e-8 at 2), and a correct engine would miss the no-op bound of 1e-3.  The
factors were chosen on the CPU from the oracle alone: the largest of 2, 3, 4 at which, on the anchor feed and on the plan feed,
no gradient key outside the two exempt groups is below 1e-4 of the largest norm (the rule of tools/fuzz_engine.py) AND every
no-op key's oracle gradient is below 1e-6 (the rule of tests/test_widths_ref_cpu.py); tests/test_variants_ref_cpu.py asserts both.

Rate and decay tables come from parameter NAMES and the slot table (rate_table, decay_table), never from the engine's head0 / rest0
arithmetic: `.bert_model.` -> lr_bert; any other key under student.news_encoder. -> lr_news_head; everything else, and what lies
between the slots -> lr; decay per adamw_ref.decay_mask."""
import numpy as np

import adamw_ref as A
import hashinit
import history_ref as HR
import widths_ref as W
from schema import state_shapes
from oracle import newsrec_oracle as O

BOOST = {"att": 4.0, "mean_ulm": 4.0, "cls_nrms": 2.0, "att_nrms_ulm": 4.0, "cls_add": 4.0}
VARIANTS = {"att": dict(pooling="att", nrms=0, ulm=False),
            "mean_ulm": dict(pooling="mean", nrms=0, ulm=True),
            "cls_nrms": dict(pooling="cls", nrms=4, ulm=False),
            "att_nrms_ulm": dict(pooling="att", nrms=4, ulm=True),
            "cls_add": dict(pooling="cls", nrms=0, ulm=False)}
NEW = ["mean_ulm", "cls_nrms", "att_nrms_ulm"]             # what the GPU file is parametrised over; "att" is the control
EMBED = ["mean_ulm", "cls_add"]                            # train_embeddings=True against torch autograd: no NRMS in the port
FLOOR = 1e-4                                               # of the largest gradient norm (tools/fuzz_engine.py)
UE = "student.user_encoder."
DENSE = O.PFX + "dense."
_MEMO = {}


def _once(key, make):
    if key not in _MEMO:
        _MEMO[key] = make()
    return _MEMO[key]


def oracle_cfg(v):
    c = VARIANTS[v]
    return dict(HR.oracle_cfg(), pooling=c["pooling"], nrms_heads=c["nrms"], user_log_mask=c["ulm"])


def engine_kwargs(v):
    """Keyword arguments of EngineConfig for the variant."""
    c = VARIANTS[v]
    return dict(HR.engine_kwargs(), pooling=c["pooling"], nrms_heads=c["nrms"], user_log_mask=c["ulm"])


def boosted(key):
    return key.endswith(".weight") and ("user_encoder." in key or key == DENSE + "weight")


def weights(v):
    """The variant's state dict (numpy), built once and never modified."""
    def make():
        c = VARIANTS[v]
        P = hashinit.init_state_dict(91, state_shapes(HR.dims(), HR.NL, HR.D, HR.T_, c["pooling"], c["nrms"]))
        return {k: (w * np.float32(BOOST[v]) if boosted(k) else w) for k, w in P.items()}
    return _once(("P", v), make)


def exempt(v, key):
    """None for a gradient held to the relative bound, else "noop" (widths_ref.NOOP: |g| < NOOP_ABS) or "zero" (pad_doc under
    user_log_mask: unused, exactly 0 on both sides)."""
    if key.endswith(W.NOOP):
        return "noop"
    if key.endswith("pad_doc") and VARIANTS[v]["ulm"]:
        return "zero"
    return None


def oracle(v, fid):
    """-> (losses [distill, target, emb], student scores, {key: gradient}, max |user|_2) of the numpy oracle for the feed at
    token level (a plan changes nothing the oracle sees), computed once."""
    def make():
        out = O.model_fwd(weights(v), oracle_cfg(v), *HR.tokens(fid))
        G = O.model_bwd(weights(v), oracle_cfg(v), out)
        un = float(np.sqrt((np.asarray(out["user"], np.float64) ** 2).sum(-1)).max())
        return np.array([out["distill_loss"], out["target_loss"], out["emb_loss"]], np.float64), out["student_score"], G, un
    return _once(("oracle", v, fid), make)


def anchor_feed():
    rec, = [r for r in HR.SCHEDULE_A if r["anchor"]]
    return rec["feed"]


def score_den(v, ref_s, un):
    """What a score error is taken relative to: max(1, |ref|max), and under NRMS max |user|_2 as well - an NRMS user vector is no
    convex combination of news vectors, so a 16-bit rounding of a candidate vector moves a logit by eps |user|_2
    (tests/test_engine_gpu.py::test_training_step_matches_reference_and_oracle, tools/fuzz_engine.py)."""
    return max(1.0, float(np.abs(ref_s).max()), un if VARIANTS[v]["nrms"] else 0.0)


def norm(g):
    return float(np.sqrt((np.asarray(g, np.float64) ** 2).sum()))


def compare_grads(v, keys, got_of, G, gtol):
    """widths_ref.compare_grads with this file's exempt(): every key against the oracle, none passed over.
    -> (worst relative L2 error, its key, [keys out of bound])."""
    worst, wk, bad = 0.0, "", []
    for k in keys:
        got, ref = np.asarray(got_of(k)), G[k]
        assert got.shape == ref.shape, (k, got.shape, ref.shape)
        how = exempt(v, k)
        if how == "noop":
            if not np.abs(got).max() < W.NOOP_ABS:
                bad.append(k)
        elif how == "zero":
            if np.abs(got).max() != 0.0 or np.abs(ref).max() != 0.0:
                bad.append(k)
        else:
            err = W.rel_l2(got, ref)
            if err > worst:
                worst, wk = err, k
            if not err < gtol:
                bad.append(k)
    return worst, wk, bad


# ---------------------------------------------------------------------------------------------------------------- tables by name
def trainable(slot):
    """[(key, offset, count, shape)] of the trainable slots, by offset."""
    return sorted([(k, o, n, shp) for k, (tr, o, n, shp) in slot.items() if tr], key=lambda x: x[1])


def rate_of(key, rates):
    """rates = (lr, lr_bert, lr_news_head)."""
    if ".bert_model." in key:
        return rates[1]
    if key.startswith(O.PFX):
        return rates[2]
    return rates[0]


def rate_table(slot, n_train, rates):
    """Per-element learning rate of the flat trainable buffer; what lies between the slots has rate `lr` (its gradient, moments and
    value are zero in training, so no update reaches it at any rate)."""
    lr = np.full(n_train, rates[0], np.float64)
    for k, o, n, _ in trainable(slot):
        lr[o:o + n] = rate_of(k, rates)
    return lr


def decay_table(slot, n_train):
    tr = trainable(slot)
    return A.decay_mask([k for k, _, _, _ in tr], [s for _, _, _, s in tr], [o for _, o, _, _ in tr], n_train)


def slot_mask(slot, n_train):
    """bool[n_train]: True inside a trainable parameter's slot."""
    m = np.zeros(n_train, bool)
    for _, o, n, _ in trainable(slot):
        assert not m[o:o + n].any()
        m[o:o + n] = True
    return m


def head_elements(slot, n_train):
    """bool[n_train]: the elements whose rate is lr_news_head - attn.* + dense.* under attention pooling, dense.* alone else."""
    m = np.zeros(n_train, bool)
    for k, o, n, _ in trainable(slot):
        if k.startswith(O.PFX) and ".bert_model." not in k:
            m[o:o + n] = True
    return m


# ---------------------------------------------------------------------------------------------------------------- torch autograd
def port_grads(v, fid):
    """embed_train_ref.port_grads for a variant with the additive user encoder: oracle/torch_port.py's model_forward, layers and
    user encoder as they are, the news encoder's pooling swapped for x[:, 0] (cls) or x.mean(1) (mean, over all L positions as
    model_bert.py:135 does) while the call runs.  -> (total loss, scores, {key: gradient}), the five embedding parameters among
    the keys; computed once."""
    def make():
        import torch.nn.functional as F
        import embed_train_ref as ER
        from oracle import torch_port as TP
        pooling = VARIANTS[v]["pooling"]
        assert not VARIANTS[v]["nrms"], "the port has no NRMS user encoder"

        def news_encoder(P, x2l, n_layers, A, eps=1e-12):
            # the port's own embedding block and layers: its news_encoder runs with att_pool standing aside (it hands the encoder's
            # output out and returns (N, H) rows for the dense call behind it, whose result is dropped)
            captured = {}
            keep_pool = TP.att_pool
            TP.att_pool = lambda x, *w, **kw: captured.setdefault("x", x)[:, 0]
            try:
                P2 = dict(P)
                for k in ("attn.att_fc1.weight", "attn.att_fc1.bias", "attn.att_fc2.weight", "attn.att_fc2.bias"):
                    P2.setdefault(TP.PFX + k, None)
                keep(P2, x2l, n_layers, A, eps)
            finally:
                TP.att_pool = keep_pool
            x = captured["x"]
            nv = x[:, 0] if pooling == "cls" else x.mean(1)
            return F.linear(nv, P[TP.PFX + "dense.weight"], P[TP.PFX + "dense.bias"])

        keep = TP.news_encoder
        if pooling != "att":
            TP.news_encoder = news_encoder
        try:
            return ER.port_grads(weights(v), oracle_cfg(v), *HR.tokens(fid))
        finally:
            TP.news_encoder = keep
    return _once(("port", v, fid), make)
