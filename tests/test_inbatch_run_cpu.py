"""CPU: the surface of --inbatch_negatives - the flag, the ids the reference feed attaches to its batches, the record in
train_state.  (The engine side is tests/test_inbatch_gpu.py, the kernels tests/test_inbatch_kernels_gpu.py.)"""
import types

import numpy as np
import pytest

import filefed_data as F
import parameters

PAT = "behaviors_np4_*.tsv"


def test_flag_parses_and_defaults_to_off():
    base = ["--mode", "train"]
    assert parameters.build_parser().parse_args(base).inbatch_negatives is False
    assert parameters.build_parser().parse_args(base + ["--inbatch_negatives", "True"]).inbatch_negatives is True
    assert parameters.build_parser().parse_args(base + ["--inbatch_negatives", "False"]).inbatch_negatives is False
    text = " ".join(parameters.build_parser().format_help().split())     # argparse wraps the text
    for word in ("(1)", "(2)", "(3)", "(4)", "(5)", "padding news", "click history", "own candidates", "data parallelism", "logged target loss"):
        assert word in text, word


@pytest.fixture(scope="module")
def shards(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("shards"))
    F.make_shards(d, F.LINE_COUNTS, seed=0)
    return d


def _loader(data_dir, inbatch, dedup=False):
    """tests/test_filefed_data_cpu.py's loader: a news table whose row r holds r, so the gathered rows ARE the indices."""
    import dataloader
    news_index = {nid: i + 1 for i, nid in enumerate(F.news_ids())}
    table = np.arange(len(news_index) + 1, dtype=np.int32).reshape(-1, 1)
    args = types.SimpleNamespace(npratio=4, user_log_length=F.USER_LOG_LENGTH, batch_size=F.BATCH, shuffle_buffer_size=10000,
                                 num_teachers=0, dedup_news=dedup)
    if inbatch is not None:
        args.inbatch_negatives = inbatch
    return dataloader.DataLoaderTrain(data_dir, PAT, args, 1, 0, 0, news_index, table, [], enable_prefetch=False,
                                      enable_shuffle=True, enable_gpu=False, resident=False)


@pytest.mark.parametrize("dedup", [False, True])
def test_reference_feed_attaches_the_ids_it_decoded(shards, dedup):
    n = 0
    for b in _loader(shards, True, dedup):
        assert len(b) == 6                                       # the 6-tuple stays the reference's
        h, c = b.ids
        assert h.dtype.is_floating_point is False and h.element_size() == 4 and c.element_size() == 4
        assert np.array_equal(h.numpy(), b[0].numpy()[..., 0]) and np.array_equal(c.numpy(), b[2].numpy()[..., 0])
        assert h.shape == (b[1].shape[0], F.USER_LOG_LENGTH) and c.shape == (b[1].shape[0], 5)
        assert dedup or b.plan is None                           # (a plan is None where it would save nothing)
        n += 1
    assert n >= 3
    for inbatch in (False, None):                                # off, or an args object from before the flag: no ids
        b = next(iter(_loader(shards, inbatch)))
        assert len(b) == 6 and b.ids is None


def test_flag_is_recorded_in_train_state():
    import run
    args = parameters.build_parser().parse_args(["--mode", "train", "--inbatch_negatives", "True"])
    on = run._train_flags(args, 2)
    assert on["inbatch_negatives"] is True and on["world"] == 2
    off = run._train_flags(parameters.build_parser().parse_args(["--mode", "train"]), 2)
    assert "inbatch_negatives" not in off                        # a run without it writes the flags it always wrote
    assert {k: v for k, v in on.items() if k != "inbatch_negatives"} == off
