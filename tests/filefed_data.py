"""Generated MIND-format inputs for the tests that feed run.py --mode train from files (no GPU needed to make them).

make_shards: behaviors_np4_<i>.tsv files in the format of tests/golden/data/behaviors_np4_*.tsv (impression id, user id, time,
history, positive, four negatives; news ids of tests/golden/data/news.tsv), with empty histories, histories longer than
--user_log_length (50: the front truncation runs) and an id the table does not hold (N999 -> row 0) among them.
expected_caps: the reference's sharding rule (Tiny-NewsRec/streaming.py:40-58, dataloader.py:61-70) restated without the
project's streaming / dataloader modules: what every rank's step count of an epoch must be.
run_py_inputs: the vocabulary, the encoder config, the teacher-embedding pickles and the PLM-NR teacher checkpoints that
run.py needs beside the behaviours files (the set-up of tests/test_dropin_gpu.py::test_run_py_train_from_mind_format_files)."""
import json
import os
import pickle
import random

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NEWS = os.path.join(GOLDEN, "data", "news.tsv")
LINE_COUNTS = (8, 12, 16, 20, 9)          # five unequal shards, 65 lines: with batch 4 the last batch of an epoch is short
BATCH = 4
USER_LOG_LENGTH = 50
UNKNOWN = "N999"                          # not in news.tsv, as in the golden behaviours files


def news_ids():
    with open(NEWS) as f:
        return [ln.split("\t")[0] for ln in f if ln.strip()]


def shard_name(i):
    return "behaviors_np4_%d.tsv" % i


def make_shards(dirname, line_counts=LINE_COUNTS, seed=0):
    """Write shard_name(i) with line_counts[i] lines into dirname (news.tsv is linked or copied beside them, where run.py looks
    for it) -> the list of paths.  Everything is a function of `seed` (a numpy RandomState of its own).  Line j of the whole
    set: j % 7 == 0 an empty history, j % 7 == 3 one of 51 .. 70 clicks, j % 7 == 5 one that holds UNKNOWN; otherwise 1 .. 50."""
    rs = np.random.RandomState(seed)
    ids = news_ids()
    os.makedirs(dirname, exist_ok=True)
    paths, j = [], 0
    for i, n in enumerate(line_counts):
        path = os.path.join(dirname, shard_name(i))
        with open(path, "w") as f:
            for _ in range(n):
                if j % 7 == 0:
                    hist = []
                elif j % 7 == 3:
                    hist = [ids[k] for k in rs.randint(0, len(ids), USER_LOG_LENGTH + 1 + int(rs.randint(0, 20)))]
                else:
                    hist = [ids[k] for k in rs.randint(0, len(ids), 1 + int(rs.randint(0, USER_LOG_LENGTH)))]
                if j % 7 == 5:
                    hist[int(rs.randint(0, len(hist)))] = UNKNOWN
                pos = ids[int(rs.randint(0, len(ids)))]
                neg = [ids[k] for k in rs.randint(0, len(ids), 4)]
                f.write("%d\tU%d\t11/15/2019 8:55:22 AM\t%s\t%s\t%s\n" % (j, j, " ".join(hist), pos, " ".join(neg)))
                j += 1
        paths.append(path)
    dst = os.path.join(dirname, "news.tsv")
    if not os.path.exists(dst):
        with open(NEWS) as src, open(dst, "w") as out:
            out.write(src.read())
    return paths


def expected_rank_batches(line_counts, world, batch, epochs):
    """[[batches of rank 0, rank 1, ...] for epoch in range(epochs)]: the file names sorted, random.Random(epoch).shuffle (what
    random.seed(epoch); random.shuffle is), rank r takes [r::world], ceil(lines / batch) batches (the last one may be short)."""
    lines = {shard_name(i): n for i, n in enumerate(line_counts)}
    out = []
    for epoch in range(epochs):
        names = sorted(lines)
        random.Random(epoch).shuffle(names)
        out.append([-(-sum(lines[f] for f in names[r::world]) // batch) for r in range(world)])
    return out


def expected_caps(line_counts, world, batch, epochs):
    """The step count of every epoch: the minimum over the ranks of expected_rank_batches."""
    return [min(per_rank) for per_rank in expected_rank_batches(line_counts, world, batch, epochs)]


def run_py_inputs(tmp_path):
    """Write vocab.txt, config.json, two teacher-embedding pickles and two PLM-NR teacher checkpoints into tmp_path
    -> (embs, ckpts, flags): the two path lists and run.py's tokenizer / config / model flags for them."""
    import hashinit
    import torch
    from helpers import FULL, state_shapes
    tmp_path = str(tmp_path)
    with open(NEWS) as f:
        rows = [ln for ln in f]
    words = sorted({w for ln in rows for w in ln.split("\t")[3].lower().split()})
    vocab = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"] + words
    with open(os.path.join(tmp_path, "vocab.txt"), "w") as f:
        f.write("\n".join(vocab) + "\n")
    with open(os.path.join(tmp_path, "config.json"), "w") as f:
        f.write(json.dumps(dict(hidden_size=768, num_attention_heads=12, intermediate_size=3072, vocab_size=len(vocab),
                                max_position_embeddings=64, type_vocab_size=2, layer_norm_eps=1e-12)))
    n_news = len(rows)
    embs, ckpts = [], []
    for i in range(2):
        p = os.path.join(tmp_path, "teacher_emb_%d.pkl" % i)
        with open(p, "wb") as f:
            pickle.dump(hashinit.hash_normal(50 + i, "temb", (n_news + 1, 256)), f)
        embs.append(p)
        sd = hashinit.init_state_dict(60 + i, {k[len("student."):]: v for k, v in state_shapes(FULL, 1, 256, 0).items()
                                               if k.startswith("student.user_encoder.")})
        ck = os.path.join(tmp_path, "teacher_%d.pt" % i)
        torch.save({"model_state_dict": {k: torch.from_numpy(v) for k, v in sd.items()}}, ck)
        ckpts.append(ck)
    flags = ["--tokenizer_name", os.path.join(tmp_path, "vocab.txt"), "--config_name", os.path.join(tmp_path, "config.json"),
             "--model_name", os.path.join(tmp_path, "none.bin"), "--allow_random_init", "True"]
    return embs, ckpts, flags
