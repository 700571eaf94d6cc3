"""Text -> tokens, and post_train_kd.py's host functions, without a GPU.

preprocess.make_tokenizer is held to (a) the table the reference made of tests/golden/data/news.tsv with its own vocabulary
(tests/golden/datapath.npz: news_combined; the vocabulary file is rebuilt from tests/golden/title_vocab.json, 30 522 lines with the
reference's tokens on their lines) and (b) tests/wordpiece_ref.py, BERT uncased tokenisation restated in plain Python, position
for position on edge texts at two widths.  Then read_corpus, token_table, load_teacher_tables, sample_indices and parse_args of
post_train_kd.py against what the notebooks' cells do, restated here."""
import functools
import json
import os
import pickle
import random
import re
import types

import numpy as np
import pytest

import post_train_kd as K
import preprocess
import wordpiece_ref as W

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NEWS = os.path.join(GOLDEN, "data", "news.tsv")


def _args(path, width=30):
    return types.SimpleNamespace(tokenizer_name=str(path), num_words_title=width)


@pytest.fixture(scope="module")
def ref_vocab(tmp_path_factory):
    """A vocabulary file of the reference's size: its tokens of title_vocab.json and its specials on their lines, fillers elsewhere."""
    with open(os.path.join(GOLDEN, "title_vocab.json")) as f:
        z = json.load(f)
    lines = ["[filler%d]" % i for i in range(z["size"])]
    for tok, i in list(z["specials"].items()) + [tuple(p) for p in z["tokens"]]:
        lines[i] = tok
    assert len(z["tokens"]) == 20 and len(set(lines)) == z["size"] == 30522
    path = tmp_path_factory.mktemp("ref_vocab") / "vocab.txt"
    path.write_text("\n".join(lines) + "\n", encoding="utf-8")
    return path


def test_news_table_equals_the_reference_table(ref_vocab):
    """All 41 x 60 entries.  With a tokenizer that lost its vocabulary the only ids are {0, 1, 2, 3}."""
    want = np.load(os.path.join(GOLDEN, "datapath.npz"))["news_combined"]
    args = _args(ref_vocab)
    news, index, cats, subcats = preprocess.read_news_bert(NEWS, args, "train")
    ids, attn, _, _ = preprocess.get_doc_input_bert(news, index, cats, subcats, args)
    got = np.concatenate([ids, attn], axis=1)
    assert got.shape == want.shape == (41, 60)
    assert np.array_equal(got, want), "ids in the table: %s, in the reference's: %s" % (np.unique(got[:, :30])[:8], np.unique(want[:, :30])[:8])


# ---------------------------------------------------------------------------------------------- make_tokenizer against wordpiece_ref
VOCAB_TEXTS = ["stocks rally after the fed cut rates", "cafe u.s.-led \"quoted\" talks, again: really?", "playing unbelievable",
               "new 中 york", "a b c d e f g h i j k l m n o p q r s t u v w x y z"]
PIECES = {"playing": ("play", "##ing"), "unbelievable": ("un", "##believ", "##able")}


def edge_texts(width):
    w = "stocks rally after the fed cut rates new york talks again really quoted led cafe a b c d e f g h i j k l m n".split()
    words = lambda n: " ".join(w[i % len(w)] for i in range(n))
    return ["", "   \t \n ", words(width - 2), words(width - 1), words(width + 5), "STOCKS Rally AFTER The Fed", "Café cafe CAFÉ",
            "u.s.-led talks", "\"quoted\" talks, again: really?", "new 中 york", "new中york", "stocks zebra rally", "playing unbelievable play",
            "x" * 120, "stocks " + "y" * 120 + " rally", "stocks\trally\nafter\r\nthe  fed", "stocks\u00a0rally\u200bfed", "stocks\x00 ral\ufffdly"]


@pytest.fixture(scope="module")
def small_vocab(tmp_path_factory):
    path = tmp_path_factory.mktemp("small_vocab") / "vocab.txt"
    vocab = W.build_vocab(str(path), VOCAB_TEXTS, pieces=PIECES)
    assert "playing" not in vocab and "##ing" in vocab and "zebra" not in vocab and vocab["[CLS]"] == 11 and vocab["[SEP]"] == 13
    return path, vocab


def _compare(tok, vocab, texts, width):
    for text in texts:
        got = tok(text, max_length=width, padding="max_length", truncation=True)
        ids, mask = W.encode(text, vocab, width)
        assert list(got["input_ids"]) == ids, (text[:40], width, list(got["input_ids"]), ids)
        assert list(got["attention_mask"]) == mask, (text[:40], width)
        assert len(ids) == width and ids[sum(mask) - 1] == vocab["[SEP]"] and ids[0] == vocab["[CLS]"]


@pytest.mark.parametrize("width", [6, 24])
def test_make_tokenizer_equals_wordpiece_ref_on_edge_texts(small_vocab, width):
    path, vocab = small_vocab
    tok = preprocess.make_tokenizer(_args(path))
    _compare(tok, vocab, edge_texts(width), width)
    # the cases are what they claim to be
    ids = lambda t: W.encode(t, vocab, 24)[0]
    assert ids("")[:3] == [11, 13, 0] and ids("   \t \n ") == ids("")
    assert ids("stocks zebra rally")[2] == vocab["[UNK]"] and ids("x" * 120)[1:3] == [vocab["[UNK]"], 13]
    assert ids("playing")[1:4] == [vocab["play"], vocab["##ing"], 13]
    assert ids("Café")[1] == vocab["cafe"] and ids("new中york")[1:4] == [vocab["new"], vocab["中"], vocab["york"]]
    assert ids("u.s.-led")[1:7] == [vocab[t] for t in ("u", ".", "s", ".", "-", "led")]
    for n, last in ((width - 2, width - 1), (width - 1, width - 1), (width + 5, width - 1)):
        got, mask = W.encode(edge_texts(width)[2 if n == width - 2 else 3 if n == width - 1 else 4], vocab, width)
        assert got[last] == 13 and sum(mask) == width


def test_make_tokenizer_equals_wordpiece_ref_on_the_golden_titles(ref_vocab):
    with open(NEWS, encoding="utf-8") as f:
        titles = [ln.rstrip("\n").split("\t")[3] for ln in f]
    tok = preprocess.make_tokenizer(_args(ref_vocab))
    _compare(tok, W.read_vocab(str(ref_vocab)), titles, 30)


def test_make_tokenizer_missing_file(tmp_path):
    with pytest.raises(FileNotFoundError, match="nowhere.txt"):
        preprocess.make_tokenizer(_args(tmp_path / "nowhere.txt"))


def test_make_tokenizer_checks_what_it_loaded(small_vocab, monkeypatch):
    """A constructor that drops the vocabulary argument (what transformers 5 does with vocab_file=) comes up with the five
    special tokens: make_tokenizer must raise, naming the file and both counts."""
    import transformers
    path, vocab = small_vocab
    real = transformers.BertTokenizer

    @functools.wraps(real)
    def dropping(*a, **kw):
        kw.pop("vocab", None)
        kw.pop("vocab_file", None)
        return real(*a, **kw)
    monkeypatch.setattr(transformers, "BertTokenizer", dropping)
    with pytest.raises(ValueError) as e:
        preprocess.make_tokenizer(_args(path))
    msg = str(e.value)
    counts = re.search(r"has (\d+) lines, the tokenizer built from it knows (\d+) tokens", msg)
    assert str(path) in msg and counts is not None, msg
    assert int(counts.group(1)) == len(vocab) and int(counts.group(2)) < 10, msg          # the specials are all it knows


def test_check_tokenizer_holds_the_specials_to_their_lines(small_vocab, tmp_path):
    """The same number of lines with [CLS] and [SEP] swapped: the size agrees, the ids do not."""
    path, vocab = small_vocab
    tok = preprocess.make_tokenizer(_args(path))
    lines = path.read_text(encoding="utf-8").split("\n")[:-1]
    lines[11], lines[13] = lines[13], lines[11]
    other = tmp_path / "swapped.txt"
    other.write_text("\n".join(lines) + "\n", encoding="utf-8")
    with pytest.raises(ValueError, match=r"\[CLS\]"):
        preprocess.check_tokenizer(tok, str(other))
    preprocess.check_tokenizer(tok, str(path))


# -------------------------------------------------------------------------------------------------------- post_train_kd.read_corpus
CORPUS = ("D0\tc\ts\tFirst title\tFirst body text\n"                          # five columns
          "D1\tc\ts\tSecond, title\tsecond body\turl\t[]\textra\n"            # more than five: the rest is ignored
          "D2\tc\ts\t\tbody of the untitled\n"                               # empty title
          "D3\tc\ts\ttitle without body\t\n"                                 # empty body
          "D4\tc\ts\tcrlf title\tcrlf body\r\n"                              # CRLF: see below
          "D5\tc\ts\tlast title\tlast body playing")                          # no newline at the end


def notebook_read(path):
    """Post-train_KD.ipynb cells 5-6."""
    with open(path, encoding="utf-8") as f:
        total_lines = f.readlines()
    titles, bodies = [], []
    for line in total_lines:
        splited = line.strip("\n").split("\t")
        titles.append(splited[3])
        bodies.append(splited[4])
    return titles, bodies


def test_read_corpus(tmp_path):
    """What the notebook's line.strip('\\n').split('\\t') gives, line by line:
      five columns          columns 3 and 4
      more than five        columns 3 and 4, the rest ignored
      empty title / body    the empty string (split keeps empty fields; strip('\\n') does not touch the tab in front of the newline)
      CRLF                  the file is opened in text mode with universal newlines: '\\r\\n' arrives as '\\n', the body has no '\\r'
      no final newline      strip has nothing to strip; the body is whole"""
    path = tmp_path / "docs.tsv"
    path.write_bytes(CORPUS.encode("utf-8"))
    titles, bodies = K.read_corpus(str(path))
    assert (titles, bodies) == notebook_read(str(path))
    assert titles == ["First title", "Second, title", "", "title without body", "crlf title", "last title"]
    assert bodies == ["First body text", "second body", "body of the untitled", "", "crlf body", "last body playing"]


def test_token_table_equals_wordpiece_ref(tmp_path):
    path = tmp_path / "docs.tsv"
    path.write_bytes(CORPUS.encode("utf-8"))
    titles, bodies = K.read_corpus(str(path))
    vocab = W.build_vocab(str(tmp_path / "vocab.txt"), titles + bodies, pieces={"playing": ("play", "##ing")}, omit=("untitled",))
    tok = preprocess.make_tokenizer(_args(tmp_path / "vocab.txt"))
    for texts, width in ((titles, 4), (bodies, 5), (titles + bodies, 16)):
        got = K.token_table(texts, tok, width)
        assert got.dtype == np.int32 and got.shape == (len(texts), 2 * width)
        want = W.table(texts, vocab, width)
        assert np.array_equal(got, want), (width, got, want)
        assert (got[:, :width][np.arange(len(texts)), got[:, width:].sum(1) - 1] == vocab["[SEP]"]).all()       # [SEP] survives truncation
    assert vocab["[UNK]"] in want[:, :16] and vocab["##ing"] in want[:, :16]


def test_load_teacher_tables(tmp_path):
    n, D, T_ = 7, 8, 3
    rs = np.random.RandomState(0)
    arrays = {}
    for i in range(T_):
        for which in ("title", "body"):
            a = rs.randn(n, D)                                             # float64, as a notebook that called .numpy() on doubles would leave
            arrays[which, i] = a
            with open(str(tmp_path / ("teacher_%s_emb_%d.pkl" % (which, i))), "wb") as f:
                pickle.dump(a, f)
    args = types.SimpleNamespace(num_teachers=T_, teacher_emb_dir=str(tmp_path), news_dim=D)
    tt, tb = K.load_teacher_tables(args, n)
    assert tt.shape == tb.shape == (T_, n, D) and tt.dtype == tb.dtype == np.float32
    for i in range(T_):
        assert np.array_equal(tt[i], arrays["title", i].astype(np.float32)) and np.array_equal(tb[i], arrays["body", i].astype(np.float32))
    with open(str(tmp_path / "teacher_body_emb_1.pkl"), "wb") as f:
        pickle.dump(arrays["body", 1][:n - 1], f)
    with pytest.raises(AssertionError, match="teacher_body_emb_1.pkl"):
        K.load_teacher_tables(args, n)


# ------------------------------------------------------------------------------------------------------ post_train_kd.sample_indices
def notebook_sample(gen, idx, n, k):
    """DistillDataset.__getitem__ (Post-train_KD.ipynb cell 8), with the generator made explicit."""
    select_list = list(range(0, idx)) + list(range(idx + 1, n))
    return [idx] + gen.sample(select_list, k)


@pytest.mark.parametrize("n,k,draws", [(7, 6, 1), (11, 3, 200)])
def test_sample_indices(n, k, draws):
    """Column 0 is the positive; the negatives are distinct, none is the positive, all lie in [0, n); over the draws every other
    document appears (rows 0 and n - 1: the two ends of the j + (j >= pos) shift); and the stream IS the notebook's: random.sample
    picks POSITIONS of its population, select_list has n - 1 entries like range(n - 1), and select_list[j] == j + (j >= idx)."""
    gen, twin = random.Random(5), random.Random(5)
    seen = {p: set() for p in range(n)}
    for _ in range(draws):
        positives = list(range(n))
        got = K.sample_indices(gen, positives, n, k)
        assert got.dtype == np.int32 and got.shape == (n, 1 + k)
        for r, pos in enumerate(positives):
            row = got[r].tolist()
            assert row[0] == pos and len(set(row)) == 1 + k and min(row) >= 0 and max(row) < n
            assert row == notebook_sample(twin, pos, n, k)
            seen[pos].update(row[1:])
    for pos in range(n):
        assert seen[pos] == set(range(n)) - {pos}, (pos, seen[pos])


def test_sample_indices_needs_k_other_documents():
    with pytest.raises(ValueError):
        K.sample_indices(random.Random(0), [0], 4, 4)
    assert K.sample_indices(random.Random(0), [], 4, 3).shape == (0, 4)


def test_parse_args_stage_0_defaults():
    a = K.parse_args(["--stage", "0"])
    assert (a.num_hidden_layers, a.bert_trainable_layer, a.num_teachers) == (12, [9, 10, 11], 0)
    a = K.parse_args(["--stage", "0", "--num_hidden_layers", "3", "--num_teachers", "4"])
    assert (a.num_hidden_layers, a.bert_trainable_layer, a.num_teachers) == (3, [9, 10, 11], 0)
    a = K.parse_args(["--stage", "0", "--bert_trainable_layer", "1", "2"])
    assert (a.num_hidden_layers, a.bert_trainable_layer) == (12, [1, 2])
    a = K.parse_args([])
    assert (a.stage, a.num_hidden_layers, a.bert_trainable_layer, a.num_teachers) == (1, 4, [2, 3], 4)
