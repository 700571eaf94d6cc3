"""CPU: the host side of --train_embeddings (EngineConfig(train_embeddings=...), the flag, the refusals) and the reference
fixture tests/golden/plmnr_embed_0.npz against the torch port's autograd."""
import json
import os

import numpy as np
import pytest

from helpers import GOLDEN, load_plmnr_case
from embed_train_ref import EMB, EMB_KEYS, WORD, port_grads, rel_l2

IFACE = json.load(open(os.path.join(GOLDEN, "interface.json")))


def _tiles(eng):
    br = sorted(eng.bucket_ranges())
    return br[0][0] == 0 and br[-1][1] == eng.n_train and all(a[1] == b[0] for a, b in zip(br, br[1:]))


def test_trainable_set_buckets_and_the_off_case():
    import engine as E
    kw = dict(n_layers=4, trainable_layers=(2, 3), num_teachers=4)
    cfg = E.EngineConfig(train_embeddings=True, **kw)
    shapes = E.param_shapes(cfg)
    assert sorted(k for k in shapes if E.is_trainable(cfg, k)) == sorted(IFACE["trainable_4layer_23"] + EMB_KEYS)
    for k in ("rel_pos_bias.weight", "pooler.dense.weight"):
        assert not E.is_trainable(cfg, E.BERT + k)
    assert not E.is_trainable(cfg, E.PFX + "bert_model.classifier.weight")
    eng = E.Engine(cfg, device="cpu", max_batch=1)        # storage layout only; no kernel is launched
    n_emb = (30522 + 512 + 2 + 2) * 768
    assert sum(v.numel() for k, v in eng.params.items() if E.is_trainable(cfg, k)) == 14841634 + n_emb
    assert eng.lo == 0 and len(eng.act) == 4 and all("qkvT" in d for d in eng.sh)
    assert _tiles(eng)
    br = eng.bucket_ranges()
    assert br[-1][0] == eng.off(WORD) == 0 and br[-1][1] >= n_emb                   # the embedding block completes last
    assert all(eng.slot[k][0] and br[-1][0] <= eng.slot[k][1] < br[-1][1] for k in EMB_KEYS)
    assert eng.build_frozen_cache(None) is False
    # off: the slot table is today's (the reference's trainable set, the same offsets as without the keyword)
    off, plain = E.Engine(E.EngineConfig(train_embeddings=False, **kw), device="cpu", max_batch=1), \
        E.Engine(E.EngineConfig(**kw), device="cpu", max_batch=1)
    assert off.slot == plain.slot and off.n_train == plain.n_train and off.lo == plain.lo == 2
    assert off.bucket_ranges() == plain.bucket_ranges() and _tiles(off)
    assert sorted(k for k, s in off.slot.items() if s[0]) == sorted(IFACE["trainable_4layer_23"])
    # a frozen layer between the embeddings and the trainable ones
    assert _tiles(E.Engine(E.EngineConfig(n_layers=2, trainable_layers=(1,), num_teachers=0, train_embeddings=True), device="cpu",
                           max_batch=1))


def test_flag_default_and_reference_flags_unchanged():
    import parameters
    a = parameters.parse_args([])
    assert a.train_embeddings is False
    for k, v in IFACE["flags"].items():
        assert getattr(a, k) == v, k
    b = parameters.parse_args("--train_embeddings True --freeze_embedding True --bert_trainable_layer 0 1".split())
    assert b.train_embeddings is True and b.freeze_embedding is True            # the latter stays inert
    import model_bert
    base = dict(vars(b), config_name=None, synthetic=True, num_student_layers=2, num_teachers=0)
    import types
    assert model_bert.engine_config_from_args(types.SimpleNamespace(**base)).train_embeddings is True
    assert model_bert.engine_config_from_args(types.SimpleNamespace(**base), is_teacher=True).train_embeddings is False
    assert model_bert.engine_config_from_args(types.SimpleNamespace(**dict(base, train_embeddings=False))).train_embeddings is False


def test_refusals():
    import engine as E
    with pytest.raises(AssertionError, match="stage1"):
        E.EngineConfig(n_layers=2, trainable_layers=(0, 1), stage1=True, user_log_length=0, train_embeddings=True)
    with pytest.raises(AssertionError, match="roberta"):
        E.EngineConfig(n_layers=2, trainable_layers=(0, 1), num_teachers=0, pos_pad_id=1, train_embeddings=True)
    with pytest.raises(AssertionError, match="trainable encoder layer"):
        E.EngineConfig(n_layers=2, trainable_layers=(), num_teachers=0, train_embeddings=True)


def test_fixture_embedding_gradients_match_the_torch_port():
    """tests/golden/plmnr_embed_0.npz (the reference's ModelBert with bert.embeddings trainable) against autograd of
    oracle/torch_port.model_forward on the same inputs, rtol 2e-4 (the oracle-vs-golden bound of this suite); row 0 of the port's
    word gradient is zeroed first - the fixture pins padding_idx: exactly zero in the reference."""
    z, P, cfg, inp = load_plmnr_case("plmnr_embed_0.npz")
    L = int(z["meta"][5])
    loss, score, G = port_grads(P, cfg, *inp)
    assert abs(loss - float(z["loss0"])) <= 2e-4 * abs(float(z["loss0"]))
    np.testing.assert_allclose(score, z["score0"], rtol=2e-4, atol=2e-5)
    names = ["student." + str(n) for n in z["grad_names"]]
    assert set(EMB_KEYS) <= set(names)
    for k in EMB_KEYS:
        n = k[len("student."):]
        assert abs(np.sqrt((G[k].astype(np.float64) ** 2).sum()) - float(z["gnorm." + n])) <= 2e-4 * float(z["gnorm." + n]), k
        scale = np.abs(z["gval." + n]).max()
        np.testing.assert_allclose(G[k].reshape(-1)[z["gidx." + n]], z["gval." + n], rtol=2e-4, atol=2e-4 * scale, err_msg=k)
    rows, want = z["word_rows"], z["word_grad_rows"]
    counts = z["word_row_counts"]
    assert rows[0] == 0 and counts[0] > 0 and list(counts[2:]) == [1, 1, 0, 0]
    assert (want[0] == 0).all() and (want[4:] == 0).all() and np.abs(want[1:4]).min(1).max() > 0
    assert rel_l2(G[WORD][rows], want) <= 2e-4
    nz = np.nonzero(np.abs(G[WORD]).max(1))[0]
    assert np.array_equal(nz, z["word_nonzero_ids"]) and 0 not in nz
    for k in EMB_KEYS[1:]:
        ref = z["grad." + k[len("student."):]]
        got = G[k][:ref.shape[0]] if ref.ndim == 2 else G[k]
        assert rel_l2(got, ref) <= 2e-4, k
    assert (z["grad." + EMB[len("student."):] + "position_embeddings.weight"][L:] == 0).all()           # rows >= L get nothing
    assert (z["grad." + EMB[len("student."):] + "token_type_embeddings.weight"][1:] == 0).all()
    assert (z["word_rows_after"][0] == P[WORD][0]).all() and (z["word_rows_after"][4:] == P[WORD][rows[4:]]).all()
    assert (z["word_rows_after"][1:4] != P[WORD][rows[1:4]]).any(1).all()
