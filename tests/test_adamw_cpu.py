"""CPU side of decoupled weight decay and the warmup / decay schedule (--weight_decay, --warmup_steps, --lr_decay_steps):
tests/adamw_ref.py is torch.optim.AdamW + lr_scheduler.LambdaLR, the decay set by name on the reference's key schema and on an
engine's slot table (gaps clear), and the flags default to off beside the unchanged reference flags."""
import json
import os

import numpy as np
import pytest
import torch

import adamw_ref as A
from conftest import GOLDEN

IFACE = json.load(open(os.path.join(GOLDEN, "interface.json")))


@pytest.mark.parametrize("ams", [True, False])
def test_adamw_ref_is_torch_adamw_with_lambda_lr(ams):
    """Eight float64 steps of torch.optim.AdamW(amsgrad=ams) with two parameter groups (decay 0.1 / no decay) under LambdaLR with
    W = 3, T = 6: the first update has lr 0, the updates at and after T have lr 0.  Bound 1e-12."""
    W, T, wd, lr, steps = 3, 6, 0.1, 1e-2, 8
    rs = np.random.RandomState(7)
    shapes = [(5, 4), (7,)]                                   # the decayed group, the exempt group
    p0 = [rs.standard_normal(s) for s in shapes]
    grads = [[rs.standard_normal(s) * 10.0 ** rs.randint(-2, 1) for s in shapes] for _ in range(steps)]
    ps = [torch.tensor(x.copy(), dtype=torch.float64, requires_grad=True) for x in p0]
    opt = torch.optim.AdamW([{"params": [ps[0]], "weight_decay": wd}, {"params": [ps[1]], "weight_decay": 0.0}],
                            lr=lr, betas=(0.9, 0.999), eps=1e-8, amsgrad=ams)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda u: A.schedule(u, W, T))
    ref = [[x.copy(), np.zeros_like(x), np.zeros_like(x), np.zeros_like(x) if ams else None] for x in p0]
    seen = []
    for s in range(steps):
        seen.append(opt.param_groups[0]["lr"])
        for p, g in zip(ps, grads[s]):
            p.grad = torch.from_numpy(g.copy())
        opt.step()
        sched.step()
        for i in range(2):
            ref[i] = list(A.adamw_step(ref[i][0], grads[s][i], ref[i][1], ref[i][2], ref[i][3], s + 1, lr * A.schedule(s, W, T),
                                       i == 0, wd))
            err = float(np.abs(ps[i].detach().numpy() - ref[i][0]).max())
            print("[adamw] ams%d step %d group %d: max|err| %.3e, err / bound %.4f" % (ams, s + 1, i, err, err / 1e-12))
            assert err <= 1e-12
    want = [lr * m for m in (0.0, 1 / 3, 2 / 3, 1.0, 2 / 3, 1 / 3, 0.0, 0.0)]
    assert np.allclose(seen, want, rtol=1e-15, atol=0.0) and seen[0] == 0.0 and seen[6] == seen[7] == 0.0
    # the decay shows: the same run without it ends elsewhere, and only in the decayed group
    plain = [p0[0].copy(), 0 * p0[0], 0 * p0[0], 0 * p0[0] if ams else None]
    for s in range(steps):
        plain = list(A.adamw_step(plain[0], grads[s][0], plain[1], plain[2], plain[3], s + 1, lr * A.schedule(s, W, T), False, wd))
    assert np.abs(plain[0] - ref[0][0]).max() > 1e-4


def test_schedule_values():
    assert [A.schedule(u, 0, 0) for u in (0, 1, 10 ** 6)] == [1.0, 1.0, 1.0]
    assert [A.schedule(u, 4, 0) for u in range(7)] == [0.0, 0.25, 0.5, 0.75, 1.0, 1.0, 1.0]           # constant with warmup
    assert [A.schedule(u, 2, 5) for u in range(8)] == [0.0, 0.5, 1.0, 2 / 3, 1 / 3, 0.0, 0.0, 0.0]
    assert [A.schedule(u, 0, 4) for u in range(6)] == [1.0, 0.75, 0.5, 0.25, 0.0, 0.0]                # decay only
    assert [A.schedule(u, 3, 3) for u in range(5)] == [0.0, 1 / 3, 2 / 3, 0.0, 0.0]                   # T - W = 0: max(1, .)
    import engine as E
    for W, T in ((0, 0), (4, 0), (2, 5), (0, 4), (3, 3), (5, 2)):
        assert [E.lr_schedule(u, W, T) for u in range(9)] == [A.schedule(u, W, T) for u in range(9)]
    assert E.lr_schedule(3, None, None) == 1.0


def test_decay_set_by_name():
    """schema.state_shapes(TINY, ...): what decays and what does not, by name; the mask over made-up slots with gaps."""
    from schema import TINY, state_shapes
    shapes = state_shapes(TINY, 2, 32, 2)
    B = "student.news_encoder.bert_model.bert."
    L0 = B + "encoder.layer.0."
    yes = ["student.news_encoder.attn.att_fc1.weight", "student.news_encoder.attn.att_fc2.weight", "student.news_encoder.dense.weight",
           "student.user_encoder.attn.att_fc1.weight", "student.user_encoder.attn.att_fc2.weight",
           "transform_matrix.0.weight", "transform_matrix.1.weight",
           L0 + "attention.self.query.weight", L0 + "attention.output.dense.weight", L0 + "intermediate.dense.weight",
           L0 + "output.dense.weight",
           B + "embeddings.word_embeddings.weight", B + "embeddings.position_embeddings.weight",
           B + "embeddings.token_type_embeddings.weight"]
    no = ["student.user_encoder.attn.att_fc2.bias", "student.news_encoder.attn.att_fc2.bias", "student.user_encoder.pad_doc",
          "student.user_encoder.attn.att_fc1.bias", "student.news_encoder.dense.bias", "transform_matrix.0.bias",
          L0 + "attention.output.LayerNorm.weight", L0 + "attention.output.LayerNorm.bias",
          L0 + "output.LayerNorm.weight", L0 + "output.LayerNorm.bias", L0 + "attention.self.query.bias",
          B + "embeddings.LayerNorm.weight", B + "embeddings.LayerNorm.bias"]
    for k in yes + no:
        assert k in shapes, k
    assert all(A.decays(k, shapes[k]) for k in yes), [k for k in yes if not A.decays(k, shapes[k])]
    assert not any(A.decays(k, shapes[k]) for k in no), [k for k in no if A.decays(k, shapes[k])]
    assert shapes["student.user_encoder.attn.att_fc2.bias"] == (1,)
    # every key falls on one side by the three-part rule, and both sides are populated
    for k, shp in shapes.items():
        assert A.decays(k, shp) == (k.endswith(".weight") and len(shp) == 2 and "LayerNorm" not in k)
    # slots that are not 32-aligned, a one-element bias between two matrices, gaps between and behind them
    names = ["a.weight", "attn.att_fc2.bias", "b.LayerNorm.weight", "c.weight", "pad_doc"]
    shp = [(3, 5), (1,), (7,), (2, 33), (1, 9)]
    offs = [2, 17, 18, 31, 100]
    mask = A.decay_mask(names, shp, offs, 130)
    want = np.zeros(130, bool)
    want[2:17] = True
    want[31:97] = True
    assert (mask == want).all()
    assert (A.unpack(A.pack(mask), 130) == mask).all() and A.pack(mask).dtype == np.uint32 and A.pack(mask).size == 5
    assert int(A.pack(mask)[0]) == sum(1 << e for e in range(32) if want[e])      # element e = bit e & 31 of word e >> 5


@pytest.mark.parametrize("train_embeddings", [False, True])
def test_engine_decay_map_is_the_mask_of_its_slot_table(train_embeddings):
    """engine.decay_words (a pure host function of the slot table) == decay_mask on the same table: per element, alignment gaps and
    the reserved rows behind att_fc1 clear, the embedding tables in the set only when they are trainable.  Nothing is allocated
    before a step asks for decay."""
    import engine as E
    cfg = E.EngineConfig(n_layers=1, trainable_layers=(0,), hidden=256, heads=4, inter=128, news_dim=32, news_query=16, user_query=20,
                         num_teachers=2, vocab=128, max_pos=64, train_embeddings=train_embeddings)
    eng = E.Engine(cfg, device="cpu", max_batch=1)
    assert eng._decay_map is None and eng.lr_scale is None
    tr = [(k, v) for k, v in eng.slot.items() if v[0]]
    mask = A.decay_mask([k for k, _ in tr], [v[3] for _, v in tr], [v[1] for _, v in tr], eng.n_train)
    words = E.decay_words(eng.slot, eng.n_train)
    assert words.dtype == np.uint32 and words.size == (eng.n_train + 31) // 32
    got = A.unpack(words, eng.n_train)
    assert (got == mask).all()
    covered = np.zeros(eng.n_train, bool)
    for _, (_, o, n, _) in tr:
        covered[o:o + n] = True
    assert (~covered).any() and not got[~covered].any()                      # the gap elements are clear
    ue = "student.user_encoder."
    o = eng.off(ue + "attn.att_fc2.bias")
    assert eng.slot[ue + "attn.att_fc2.bias"][2] == 1 and not got[o] and got[o - 1 - 32] and not got[o - 1]     # [fc2.weight | pad_doc | bias]
    assert o % 32 != 0 or eng.off(ue + "pad_doc") % 32 != 0                  # slots are not word-aligned: per-element granularity
    emb = E.BERT + "embeddings.word_embeddings.weight"
    assert eng.slot[emb][0] == train_embeddings
    if train_embeddings:
        o, n = eng.slot[emb][1], eng.slot[emb][2]
        assert got[o:o + n].all()
        o = eng.off(E.BERT + "embeddings.LayerNorm.weight")
        assert not got[o:o + 256].any()
    assert not any(k.startswith("teachers.") for k, _ in tr)
    assert mask.sum() == sum(v[2] for k, v in tr if A.decays(k, v[3]))
    second = E.Engine(cfg, device="cpu", max_batch=1, share=eng)
    assert second._clip_owner is eng and second._decay_map is None and eng._decay_map is None


def test_flags_default_to_off_and_reference_flags_keep_their_defaults():
    import parameters
    import post_train_kd
    a = vars(parameters.parse_args([]))
    assert a["weight_decay"] == 0.0 and isinstance(a["weight_decay"], float)
    assert a["warmup_steps"] == 0 and a["lr_decay_steps"] == 0 and isinstance(a["warmup_steps"], int)
    for k, v in IFACE["flags"].items():
        assert a[k] == v, "--%s default %r != reference %r" % (k, a[k], v)
    assert not {"weight_decay", "warmup_steps", "lr_decay_steps"} & set(IFACE["flags"])
    b = parameters.parse_args(["--weight_decay", "0.01", "--warmup_steps", "100", "--lr_decay_steps", "1000"])
    assert (b.weight_decay, b.warmup_steps, b.lr_decay_steps) == (0.01, 100, 1000)
    c = post_train_kd.parse_args([])
    assert (c.weight_decay, c.warmup_steps, c.lr_decay_steps) == (0.0, 0, 0)
    d = post_train_kd.parse_args(["--weight_decay", "0.1", "--warmup_steps", "7", "--lr_decay_steps", "9"])
    assert (d.weight_decay, d.warmup_steps, d.lr_decay_steps) == (0.1, 7, 9)
    from model_bert import TnrAdam
    o = TnrAdam(None, 1e-4)
    assert (o.weight_decay, o.warmup_steps, o.lr_decay_steps) == (0.0, 0, 0)
