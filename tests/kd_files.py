"""Generated inputs for the tests that feed post_train_kd.py from files (no GPU needed to make them), and the script's
documented sampling rule restated without importing it.  In the manner of tests/filefed_data.py.

write_inputs(dir) -> flags: docs_filter.tsv (N_DOCS = 27 documents: odd, so that two ranks' shares of an epoch differ by one, and
no multiple of the batch of 4), vocab.txt for it (wordpiece_ref.build_vocab: ids not dense, specials off lines 0-4, `playing` /
`markets` present as pieces only, `zyzzyva` absent) and config.json (hidden 256, 4 heads, inter 512, max_position_embeddings 64 -
below the body length of 72, so post_train_kd._model_dims' max(..., max_body_len) decides the table's length - and both dropout
probabilities 0.1).  --model_name names a file that does not exist (--allow_random_init True).
  document EMPTY_TITLE has an empty title, EMPTY_BODY an empty body, LONG_TITLE a title of more than 12 wordpieces, LONG_BODY a
  body of more than 72; every other title has 3 .. 9 words, every other body 20 .. 60.
Shapes: titles of 12 (the short attention kernels), bodies of 72 (the long attention kernels at 96 rows, the chunked pooling with
an 8-token last chunk, as in tests/stage1_history_ref.py), 1 + 3 documents a sample, batch 4.

expected_indices(seed, rank, world, epoch, n_docs, batch, k, steps): what the script documents -
  order = list(range(n_docs)); random.Random(seed + epoch).shuffle(order)      the same on every rank
  order[rank::world]                                                           this rank's share
  (n_docs // world) // batch steps an epoch, batch positives each, in that order
  negatives: for each positive random.sample(range(n_docs - 1), k) of the generator random.seed(seed + rank) gives, one stream
  through all epochs of a run; j -> j + (j >= positive)."""
import json
import os
import random

import numpy as np

import wordpiece_ref as W

N_DOCS = 27
BATCH = 4
K = 3
LT, LB = 12, 72
HIDDEN, HEADS, INTER, MAX_POS_CFG, NEWS_DIM, QUERY = 256, 4, 512, 64, 256, 200
EMPTY_TITLE, EMPTY_BODY, LONG_TITLE, LONG_BODY = 5, 9, 2, 3
SEED = 7          # chosen (test_kd_files_cpu.py asserts it) so that step 1 at world 1 holds EMPTY_TITLE and EMPTY_BODY
WORDS = ("stocks fed rate cut markets rally storm coast team wins final open signals lower after hits playing play city council "
         "votes budget new park river bridge closed repairs school board meets tuesday local bakery award").split()
PIECES = {"playing": ("play", "##ing"), "markets": ("market", "##s")}
OMIT = ("zyzzyva",)


def corpus():
    """-> (titles, bodies): N_DOCS strings each, a function of nothing."""
    rs = random.Random(4242)
    draw = lambda n: " ".join(rs.choice(WORDS) for _ in range(n))
    titles = [draw(rs.randint(3, 9)) for _ in range(N_DOCS)]
    bodies = [draw(rs.randint(20, 60)) for _ in range(N_DOCS)]
    titles[EMPTY_TITLE] = ""
    bodies[EMPTY_BODY] = ""
    titles[LONG_TITLE] = "Playing markets, again: " + draw(11) + " zyzzyva"
    bodies[LONG_BODY] = draw(70) + ". Café u.s.-led " + draw(10)
    titles[7] = "Fed signals zyzzyva RATE cut; markets rally"
    bodies[11] = draw(15) + " zyzzyva playing " + draw(15)
    return titles, bodies


def write_inputs(dirname):
    """Write docs_filter.tsv, vocab.txt and config.json into dirname -> post_train_kd.py's flags for them (without --stage,
    --save_dir, --teacher_emb_dir, --num_teachers and the optimiser's)."""
    dirname = str(dirname)
    os.makedirs(dirname, exist_ok=True)
    titles, bodies = corpus()
    with open(os.path.join(dirname, "docs_filter.tsv"), "w", encoding="utf-8") as f:
        for i, (t, b) in enumerate(zip(titles, bodies)):
            f.write("D%d\tcat%d\tsub%d\t%s\t%s\n" % (i, i % 3, i % 5, t, b))
    vocab = W.build_vocab(os.path.join(dirname, "vocab.txt"), titles + bodies, pieces=PIECES, omit=OMIT)
    with open(os.path.join(dirname, "config.json"), "w") as f:
        f.write(json.dumps(dict(hidden_size=HIDDEN, num_attention_heads=HEADS, intermediate_size=INTER, vocab_size=len(vocab),
                                max_position_embeddings=MAX_POS_CFG, type_vocab_size=2, layer_norm_eps=1e-12,
                                hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1)))
    return ["--corpus_path", os.path.join(dirname, "docs_filter.tsv"), "--tokenizer_name", os.path.join(dirname, "vocab.txt"),
            "--config_name", os.path.join(dirname, "config.json"), "--model_name", os.path.join(dirname, "none.bin"),
            "--allow_random_init", "True", "--max_title_len", str(LT), "--max_body_len", str(LB), "--npratio", str(K),
            "--batch_size", str(BATCH), "--news_dim", str(NEWS_DIM), "--seed", str(SEED), "--log_steps", "1"]


def tables(dirname):
    """The token tables of the corpus by wordpiece_ref (the script lowercases the text itself first): (27, 24) and (27, 144)."""
    vocab = W.read_vocab(os.path.join(str(dirname), "vocab.txt"))
    titles, bodies = corpus()
    return W.table([t.lower() for t in titles], vocab, LT), W.table([b.lower() for b in bodies], vocab, LB)


def engine_dims(dirname):
    """Keyword arguments of Stage1Engine that the flags of write_inputs stand for (without layers, teachers, device, dtype)."""
    n_vocab = len(W.read_vocab(os.path.join(str(dirname), "vocab.txt")))
    return dict(npratio=K, title_len=LT, body_len=LB, batch=BATCH, hidden=HIDDEN, heads=HEADS, inter=INTER, vocab=n_vocab,
                max_pos=max(MAX_POS_CFG, LB), type_vocab=2, ln_eps=1e-12, news_dim=NEWS_DIM, news_query=QUERY)


def steps_per_epoch(n_docs, world, batch):
    return (n_docs // world) // batch


def shuffled(seed, epoch, n_docs):
    order = list(range(n_docs))
    random.Random(seed + epoch).shuffle(order)
    return order


def expected_indices(seed, rank, world, epoch, n_docs, batch, k, steps=None):
    """-> list of `steps` (batch, 1 + k) int32 arrays: the index batches of epoch `epoch` on rank `rank` (the negatives' generator
    is run through the epochs before it first: one stream per process)."""
    gen = random.Random(seed + rank)
    out = []
    for ep in range(epoch + 1):
        mine = shuffled(seed, ep, n_docs)[rank::world]
        n = steps_per_epoch(n_docs, world, batch) if steps is None else steps
        out = []
        for s in range(n):
            idx = np.empty((batch, 1 + k), dtype=np.int32)
            for r, pos in enumerate(mine[s * batch:(s + 1) * batch]):
                neg = gen.sample(range(n_docs - 1), k)
                idx[r, 0] = pos
                idx[r, 1:] = [j + (j >= pos) for j in neg]
            out.append(idx)
    return out
