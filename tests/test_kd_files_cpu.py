"""tests/kd_files.py without a GPU: the generated corpus is what its docstring says, and expected_indices is the rule
post_train_kd.py documents (one shuffle per epoch shared by the ranks, a strided share, floor step counts, per-rank negatives)."""
import random

import numpy as np
import pytest

import kd_files as F
import wordpiece_ref as W


def test_corpus_and_tables(tmp_path):
    flags = F.write_inputs(tmp_path)
    assert flags[flags.index("--seed") + 1] == str(F.SEED)
    with open(str(tmp_path / "docs_filter.tsv"), encoding="utf-8") as f:
        lines = f.readlines()
    assert len(lines) == F.N_DOCS == 27 and F.N_DOCS % 2 == 1 and F.N_DOCS % F.BATCH
    vocab = W.read_vocab(str(tmp_path / "vocab.txt"))
    titles, bodies = F.corpus()
    assert titles[F.EMPTY_TITLE] == "" and bodies[F.EMPTY_BODY] == ""
    assert len(W.tokens(titles[F.LONG_TITLE], vocab)) > F.LT - 2 and len(W.tokens(bodies[F.LONG_BODY], vocab)) > F.LB - 2
    t, b = F.tables(tmp_path)
    assert t.shape == (27, 2 * F.LT) and b.shape == (27, 2 * F.LB) and t.dtype == b.dtype == np.int32
    assert t[F.EMPTY_TITLE, F.LT:].sum() == 2 and b[F.EMPTY_BODY, F.LB:].sum() == 2                 # [CLS] [SEP]
    assert t[F.LONG_TITLE, F.LT:].sum() == F.LT and t[F.LONG_TITLE, F.LT - 1] == vocab["[SEP]"]
    assert b[F.LONG_BODY, F.LB:].sum() == F.LB and b[F.LONG_BODY, F.LB - 1] == vocab["[SEP]"]
    lens = b[:, F.LB:].sum(1)
    assert (lens > 64).sum() >= 1 and (lens <= 64).sum() >= 20                                        # both sides of the pooling chunk
    assert vocab["[UNK]"] in t[:, :F.LT] and vocab["##ing"] in t[:, :F.LT] and "playing" not in vocab
    assert max(vocab.values()) + 1 == len(vocab) and F.engine_dims(tmp_path)["max_pos"] == F.LB > F.MAX_POS_CFG


def test_first_step_holds_both_empty_documents():
    idx = F.expected_indices(F.SEED, 0, 1, 0, F.N_DOCS, F.BATCH, F.K, 1)[0]
    assert F.EMPTY_BODY in idx[:, 0] and F.EMPTY_TITLE in idx          # the body is the positive's; a title may be anybody's


@pytest.mark.parametrize("world", [1, 2, 3])
def test_expected_indices_is_the_documented_rule(world):
    seed, n, B, k = F.SEED, F.N_DOCS, F.BATCH, F.K
    steps = {1: 6, 2: 3, 3: 2}[world]
    assert F.steps_per_epoch(n, world, B) == steps == (n // world) // B
    for epoch in (0, 1):
        order = list(range(n))
        random.Random(seed + epoch).shuffle(order)
        per_rank = [F.expected_indices(seed, r, world, epoch, n, B, k) for r in range(world)]
        pos = [np.concatenate([i[:, 0] for i in batches]).tolist() for batches in per_rank]
        assert all(len(batches) == steps for batches in per_rank)
        flat = [p for ps in pos for p in ps]
        assert len(set(flat)) == len(flat) == world * steps * B                                        # disjoint
        inter = [pos[j % world][j // world] for j in range(world * steps * B)]
        assert inter == order[:world * steps * B]                                                      # a prefix, interleaved
        for r, batches in enumerate(per_rank):
            for i in batches:
                assert i.dtype == np.int32 and i.shape == (B, 1 + k)
                for row in i.tolist():
                    assert len(set(row)) == 1 + k and 0 <= min(row) and max(row) < n
        if world > 1:                                                                                  # per-rank negative streams
            assert not np.array_equal(per_rank[0][0][:, 1:], per_rank[1][0][:, 1:])
    # the negatives' generator is one stream through the epochs of a process
    gen = random.Random(seed + 0)
    for epoch in (0, 1):
        want = F.expected_indices(seed, 0, world, epoch, n, B, k)
        for i in want:
            for row in i:
                neg = gen.sample(range(n - 1), k)
                assert row[1:].tolist() == [j + (j >= row[0]) for j in neg]
