"""news.tsv -> news_index and the padded token tables (layout of Tiny-NewsRec/preprocess.py:15-66), TF-free.

Tokenisation itself is one-off host work and out of scope for kernels: any callable
`tokenizer(text, max_length=, padding="max_length", truncation=True) -> {"input_ids", "attention_mask"}` works,
by default transformers' BertTokenizer on the reference's vocab file.  What matters downstream is the layout:
news ids are numbered 1..n in file order, row 0 of every table is the all-zero pad news, tables are int32."""
import numpy as np


SPECIALS = ("[PAD]", "[UNK]", "[CLS]", "[SEP]")


def read_vocab(path):
    """The vocabulary file as BertTokenizer's load_vocab reads it: one token per line, the id is the line's number."""
    with open(path, "r", encoding="utf-8") as fh:
        return [line.rstrip("\n") for line in fh]


def make_tokenizer(args):
    """BertTokenizer on the vocabulary file --tokenizer_name, under either spelling of the constructor's parameter: `vocab_file`
    (a path; transformers 4) or `vocab` (transformers 5, handed the {token: id} dict read here) - a keyword the constructor does
    not know disappears into its **kwargs and leaves a tokenizer of the five special tokens, for which every word is [UNK].
    Whatever was built is then held to the file: as many entries as the file has lines, the four specials the tables rely
    on at the ids of their lines."""
    import inspect
    import os

    from transformers import BertTokenizer
    path = args.tokenizer_name
    if not os.path.isfile(path):
        raise FileNotFoundError("--tokenizer_name %s does not exist" % path)
    tokens = read_vocab(path)
    names = inspect.signature(BertTokenizer).parameters
    if "vocab_file" in names:
        tok = BertTokenizer(vocab_file=path, do_lower_case=True)
    elif "vocab" in names:
        tok = BertTokenizer(vocab={t: i for i, t in enumerate(tokens)}, do_lower_case=True)
    else:
        raise RuntimeError("BertTokenizer takes neither vocab_file nor vocab: %s" % ", ".join(names))
    check_tokenizer(tok, path, tokens)
    return tok


def check_tokenizer(tok, path, tokens=None):
    """Raise unless `tok` holds the vocabulary file `path`: len(tok) lines, [PAD] / [UNK] / [CLS] / [SEP] at their lines' ids."""
    tokens = read_vocab(path) if tokens is None else tokens
    if len(tok) != len(tokens):
        raise ValueError("--tokenizer_name %s has %d lines, the tokenizer built from it knows %d tokens"
                         % (path, len(tokens), len(tok)))
    for name in SPECIALS:
        want = tokens.index(name) if name in tokens else None
        got = tok.convert_tokens_to_ids(name)
        if want is None or got != want:
            raise ValueError("--tokenizer_name %s (%d lines, %d tokens loaded): %s is on line %s of the file, the tokenizer gives "
                             "it id %s" % (path, len(tokens), len(tok), name, want, got))


def _number(table, key):
    return table.setdefault(key, len(table) + 1)


def read_news_bert(news_path, args, mode="train", tokenizer=None):
    assert mode in ("train", "test"), "Wrong mode!"
    encode = tokenizer or make_tokenizer(args)
    width = args.num_words_title
    news, news_index, categories, subcategories = {}, {}, {}, {}
    with open(news_path, "r", encoding="utf-8") as fh:
        for row in fh:
            doc_id, cat, subcat, title = row.rstrip("\n").split("\t")[:4]
            _number(news_index, doc_id)
            tokens = encode(title.lower(), max_length=width, padding="max_length", truncation=True)
            news.setdefault(doc_id, [tokens, cat, subcat])
            if mode == "train":
                _number(categories, cat)
                _number(subcategories, subcat)
    return (news, news_index, categories, subcategories) if mode == "train" else (news, news_index)


def get_doc_input_bert(news, news_index, category_dict, subcategory_dict, args):
    rows, width = len(news) + 1, args.num_words_title
    ids = np.zeros((rows, width), dtype="int32")
    attn = np.zeros((rows, width), dtype="int32")
    cats = np.zeros(rows, dtype="int32")
    subcats = np.zeros(rows, dtype="int32")
    for doc_id, (tokens, cat, subcat) in news.items():
        r = news_index[doc_id]
        ids[r], attn[r] = tokens["input_ids"], tokens["attention_mask"]
        cats[r], subcats[r] = category_dict.get(cat, 0), subcategory_dict.get(subcat, 0)
    return ids, attn, cats, subcats
