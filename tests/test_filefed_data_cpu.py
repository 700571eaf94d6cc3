"""The generated shards of tests/filefed_data.py and the host half of run.py's file-fed --resume claim (no GPU).

expected_caps is a restatement of the reference's sharding rule that imports neither streaming nor dataloader; here it is held
against both.  The GPU cases of tests/test_run_dp_resume_gpu.py rest on two facts that are checked here, not assumed: epoch 0 and
epoch 1 of these shards differ (files per rank, step cap, line order, label draws), so a resume that forgets the epoch counter
cannot pass; and a FRESH loader told `epoch = 0` yields as its next epoch exactly the batches a loader that went through epoch 0
yields as its second - the shard assignment, the line shuffle and the label stream (Python's global `random`, re-seeded by the
epoch's get_worker_files) all follow the epoch number alone.  A failure of the GPU resume cases with this file passing is the
engine's or run.py's; with this file failing it is the loader's."""
import os
import random
import types

import numpy as np
import pytest

import filefed_data as F

PAT = "behaviors_np4_*.tsv"
WORLD = 2


@pytest.fixture(scope="module")
def shards(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("shards"))
    F.make_shards(d, F.LINE_COUNTS, seed=0)
    return d


def _loader(data_dir, rank=0, world=1, prefetch=False):
    """DataLoaderTrain on the host, as run.py builds it (enable_shuffle=True, the default --shuffle_buffer_size), with a news
    table whose row r holds r: the gathered rows ARE the indices.  -> (loader, the impression ids of every batch it decodes)."""
    import dataloader
    news_index = {nid: i + 1 for i, nid in enumerate(F.news_ids())}
    table = np.arange(len(news_index) + 1, dtype=np.int32).reshape(-1, 1)
    args = types.SimpleNamespace(npratio=4, user_log_length=F.USER_LOG_LENGTH, batch_size=F.BATCH, shuffle_buffer_size=10000,
                                 num_teachers=0)
    dl = dataloader.DataLoaderTrain(data_dir, PAT, args, world, rank, 0, news_index, table, [], enable_prefetch=prefetch,
                                    enable_shuffle=True, enable_gpu=False, resident=False)
    seen, decode = [], dl.decode

    def recording(batch):
        seen.append([int(ln.split(b"\t")[0]) for ln in batch])
        return decode(batch)
    dl.decode = recording
    return dl, seen


def _epoch(dl):
    """One epoch -> [(hist, mask, cand, label) numpy arrays per batch]"""
    return [tuple(np.asarray(x.numpy()).copy() for x in b[:4]) for b in dl]


def _same(a, b):
    return len(a) == len(b) and all(len(x) == len(y) and all(np.array_equal(u, v) for u, v in zip(x, y)) for x, y in zip(a, b))


def test_shards_have_the_format_and_the_edge_cases(shards):
    ids = set(F.news_ids())
    assert len(ids) == 40 and F.UNKNOWN not in ids
    n_empty = n_long = n_unknown = 0
    seen = []
    for i, n in enumerate(F.LINE_COUNTS):
        with open(os.path.join(shards, F.shard_name(i))) as f:
            rows = f.read().split("\n")
        assert rows[-1] == "" and len(rows) == n + 1
        for ln in rows[:-1]:
            iid, uid, _, hist, pos, neg = ln.split("\t")
            seen.append(int(iid))
            assert uid == "U" + iid and pos in ids and len(neg.split()) == 4 and set(neg.split()) <= ids
            h = hist.split()
            assert set(h) <= ids | {F.UNKNOWN}
            n_empty += not h
            n_long += len(h) > F.USER_LOG_LENGTH
            n_unknown += F.UNKNOWN in h
    assert seen == list(range(sum(F.LINE_COUNTS)))
    assert n_empty >= 2 and n_long >= 2 and n_unknown >= 2
    # the same seed writes the same bytes, another seed other ones
    again, other = shards + "_again", shards + "_other"
    F.make_shards(again, F.LINE_COUNTS, seed=0)
    F.make_shards(other, F.LINE_COUNTS, seed=1)
    read = lambda d: [open(os.path.join(d, F.shard_name(i)), "rb").read() for i in range(len(F.LINE_COUNTS))]
    assert read(again) == read(shards) and read(other) != read(shards)
    # the decode of such lines: front truncation keeps the LAST 50 clicks, the unknown id is row 0 with its mask at 1
    dl, _ = _loader(shards)
    long_ = [F.news_ids()[k % 40] for k in range(60)]
    h, m, c, y = dl.decode([("0\tU0\tt\t%s\tN1\tN2 N3 N4 N5" % " ".join(long_)).encode(),
                            b"1\tU1\tt\t\tN1\tN2 N3 N4 N5", ("2\tU2\tt\tN7 %s N9\tN1\tN2 N3 N4 N5" % F.UNKNOWN).encode()])
    assert h[0].tolist() == [dl.news_index[x] for x in long_[-50:]] and m[0].sum() == 50
    assert h[1].sum() == 0 and m[1].sum() == 0
    assert h[2, -3:].tolist() == [7, 0, 9] and m[2].tolist() == [0.0] * 47 + [1.0] * 3


def test_expected_caps_is_the_loaders_rule(shards):
    import streaming
    stat = streaming.get_stat(shards, PAT)
    assert sorted(stat.values()) == sorted(F.LINE_COUNTS)
    per_rank = F.expected_rank_batches(F.LINE_COUNTS, WORLD, F.BATCH, 3)
    caps = F.expected_caps(F.LINE_COUNTS, WORLD, F.BATCH, 3)
    # the figures the GPU cases are built on: 44 / 21 lines in epoch 0, 37 / 28 in epoch 1
    assert per_rank[:2] == [[11, 6], [10, 7]] and caps[:2] == [6, 7]
    for epoch in range(3):
        mine = []
        for r in range(WORLD):
            dl, _ = _loader(shards, r, WORLD)
            dl.epoch = epoch - 1
            mine.append(dl.next_epoch_batches(stat))
            assert dl.next_epoch_batches(None) == mine[-1]           # counted from the files themselves
            files = streaming.shard_files(shards, r, WORLD, PAT, True, epoch)
            assert -(-sum(stat[f] for f in files) // F.BATCH) == mine[-1]
        assert mine == per_rank[epoch] and min(mine) == caps[epoch]
    # one rank: every line, the last batch short
    assert F.expected_caps(F.LINE_COUNTS, 1, F.BATCH, 2) == [17, 17]


@pytest.mark.parametrize("rank,world", [(0, 1), (0, 2), (1, 2)])
def test_epoch_0_and_epoch_1_differ(shards, rank, world):
    """The precondition of the resume cases: what the epoch counter selects is visible in the batches."""
    dl, seen = _loader(shards, rank, world)
    random.seed(99)                                        # whatever state the process is in: the epoch re-seeds it
    e0 = _epoch(dl)
    ids0 = list(seen)
    del seen[:]
    e1 = _epoch(dl)
    ids1 = list(seen)
    per_rank = F.expected_rank_batches(F.LINE_COUNTS, world, F.BATCH, 2)
    assert [len(e0), len(e1)] == [per_rank[0][rank], per_rank[1][rank]]
    flat = lambda ids: [i for b in ids for i in b]
    assert flat(ids0) != flat(ids1)                                          # line order
    if world == 1:
        assert sorted(flat(ids0)) == sorted(flat(ids1)) == list(range(sum(F.LINE_COUNTS)))
        assert [len(b) for b in ids0] == [4] * 16 + [1]                      # the short last batch
    else:
        assert set(flat(ids0)) != set(flat(ids1))                            # another file set
    assert any(a[3].shape != b[3].shape or not np.array_equal(a[3], b[3]) for a, b in zip(e0, e1))      # label vectors
    assert all(int(y.min()) >= 0 and int(y.max()) <= 4 for _, _, _, y in e0 + e1)


@pytest.mark.parametrize("prefetch", [False, True], ids=["in_line", "producer_thread"])
@pytest.mark.parametrize("rank,world", [(0, 1), (1, 2)])
def test_a_fresh_loader_at_epoch_0_replays_the_second_epoch(shards, rank, world, prefetch):
    """What run.py --resume does to the loader (loader.epoch = first_epoch - 1) against the loader of the uninterrupted run."""
    straight, seen_s = _loader(shards, rank, world, prefetch)
    random.seed(5)
    first = _epoch(straight)
    n_first = len(seen_s)
    second = _epoch(straight)
    straight.join()
    resumed, seen_r = _loader(shards, rank, world, prefetch)
    random.seed(6)                                         # a fresh process starts its generator elsewhere
    resumed.epoch = 0
    replay = _epoch(resumed)
    resumed.join()
    assert seen_r == seen_s[n_first:]                      # the same lines in the same batches
    assert _same(second, replay)
    assert not _same(first, replay)
    # and two fresh loaders agree on epoch 0: a run is reproducible from process to process
    other, _ = _loader(shards, rank, world, prefetch)
    random.seed(7)
    assert _same(first, _epoch(other))
    other.join()


@pytest.mark.parametrize("prefetch", [False, True], ids=["in_line", "producer_thread"])
def test_rows_gathered_on_the_host_carry_the_resident_feeds_plan(shards, prefetch):
    """--resident_tables False under --dedup_news: the reference's 6-tuple, and on it (RowBatch.plan) the de-duplication plan
    the resident feed builds from the same indices - what lets both feeds encode the same rows.  The engine takes each distinct
    news' token row from its first slot (order[seg[i]]): that slot does hold news uniq[i]."""
    from dedup import build_plan
    dl, _ = _loader(shards, prefetch=prefetch)
    plain = _epoch(dl)
    dl.join()
    dl, _ = _loader(shards, prefetch=prefetch)
    dl.dedup = True
    n_plans = 0
    for batch, (h, m, c, y) in zip(dl, plain):
        assert len(batch) == 6 and all(np.array_equal(a.numpy(), b) for a, b in zip(batch[:4], (h, m, c, y)))
        want = build_plan(h[..., 0], c[..., 0])
        assert (batch.plan is None) == (want is None)
        if want is None:
            assert h.shape[0] == 1                            # the short last batch: nothing to save
            continue
        n_plans += 1
        for k in ("uniq", "inv", "order", "seg"):
            assert np.array_equal(getattr(batch.plan, k), getattr(want, k)), k
        assert (batch.plan.n_enc, batch.plan.n_unique, batch.plan.n_slots) == (want.n_enc, want.n_unique, want.n_slots)
        p = batch.plan
        slots = np.concatenate([h.reshape(-1), c.reshape(-1)])
        assert p.n_enc == 64 and p.n_slots == slots.size == 220 and np.array_equal(p.uniq[p.inv], slots)
        assert np.array_equal(slots[p.order[p.seg[:p.n_unique]]], p.uniq[:p.n_unique]) and not p.uniq[p.n_unique:].any()
    dl.join()
    assert n_plans == 16
