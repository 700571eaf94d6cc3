"""BERT uncased tokenisation restated in plain Python (no transformers, no tokenizers), and a vocabulary-file builder.

What `BertTokenizer(vocab, do_lower_case=True)(text, max_length=w, padding="max_length", truncation=True)` stands for
(Devlin et al.'s tokenization.py: BasicTokenizer + WordpieceTokenizer):
  1. clean: drop U+0000, U+FFFD and control characters (category C* except tab / newline / carriage return); every whitespace
     character (space, tab, newline, carriage return, category Zs) becomes one space;
  2. a space on either side of every CJK ideograph;
  3. lowercase, then strip accents: NFD, drop category Mn;
  4. split on whitespace; split every punctuation character (ASCII 33-47, 58-64, 91-96, 123-126, or category P*) off as a word
     of its own;
  5. WordPiece per word: greedy longest match first, continuations carry "##"; a word of more than 100 characters, or one where
     some position has no match, is [UNK] as a whole;
  6. [CLS] pieces [SEP] with the pieces cut to max_length - 2 ([SEP] stays last), padded with [PAD]; the attention mask is 1 on
     everything but the padding.

read_vocab(path) -> {token: id} (one token per line, id = line number).  encode(text, vocab, width) -> (ids, mask).
table(texts, vocab, width) -> (n, 2 width) int32 [ids | mask], the layout of post_train_kd.token_table.
build_vocab(path, texts, pieces=, omit=) writes a vocabulary file for `texts` whose ids are NOT dense and whose specials do not
sit on lines 0-4."""
import unicodedata

import numpy as np

MAX_WORD_CHARS = 100
PAD, UNK, CLS, SEP, MASK = "[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"


def _is_whitespace(ch):
    return ch in " \t\n\r" or unicodedata.category(ch) == "Zs"


def _is_control(ch):
    return ch not in "\t\n\r" and unicodedata.category(ch).startswith("C")


def _is_punctuation(ch):
    cp = ord(ch)
    if 33 <= cp <= 47 or 58 <= cp <= 64 or 91 <= cp <= 96 or 123 <= cp <= 126:
        return True
    return unicodedata.category(ch).startswith("P")


def _is_cjk(ch):
    cp = ord(ch)
    return (0x4E00 <= cp <= 0x9FFF or 0x3400 <= cp <= 0x4DBF or 0x20000 <= cp <= 0x2A6DF or 0x2A700 <= cp <= 0x2B73F
            or 0x2B740 <= cp <= 0x2B81F or 0x2B820 <= cp <= 0x2CEAF or 0xF900 <= cp <= 0xFAFF or 0x2F800 <= cp <= 0x2FA1F)


def basic_tokens(text):
    """Steps 1-4: the words WordPiece is applied to."""
    out = []
    for ch in text:
        if ord(ch) in (0, 0xFFFD) or _is_control(ch):
            continue
        if _is_whitespace(ch):
            out.append(" ")
        elif _is_cjk(ch):
            out.append(" " + ch + " ")
        else:
            out.append(ch)
    text = "".join(out).lower()
    text = "".join(ch for ch in unicodedata.normalize("NFD", text) if unicodedata.category(ch) != "Mn")
    words = []
    for chunk in text.split():
        cur = ""
        for ch in chunk:
            if _is_punctuation(ch):
                if cur:
                    words.append(cur)
                words.append(ch)
                cur = ""
            else:
                cur += ch
        if cur:
            words.append(cur)
    return words


def wordpiece(word, vocab):
    """Step 5 for one word -> list of tokens."""
    if len(word) > MAX_WORD_CHARS:
        return [UNK]
    pieces, start = [], 0
    while start < len(word):
        end = len(word)
        while end > start:
            piece = ("##" if start else "") + word[start:end]
            if piece in vocab:
                break
            end -= 1
        if end == start:
            return [UNK]
        pieces.append(piece)
        start = end
    return pieces


def tokens(text, vocab):
    return [p for w in basic_tokens(text) for p in wordpiece(w, vocab)]


def encode(text, vocab, width):
    """Step 6 -> (ids, mask), two lists of `width` ints."""
    ids = [vocab[CLS]] + [vocab[t] for t in tokens(text, vocab)][:width - 2] + [vocab[SEP]]
    n = len(ids)
    return ids + [vocab[PAD]] * (width - n), [1] * n + [0] * (width - n)


def table(texts, vocab, width):
    out = np.zeros((len(texts), 2 * width), dtype=np.int32)
    for i, text in enumerate(texts):
        ids, mask = encode(text, vocab, width)
        out[i, :width], out[i, width:] = ids, mask
    return out


def read_vocab(path):
    with open(path, encoding="utf-8") as f:
        return {ln.rstrip("\n"): i for i, ln in enumerate(f)}


def build_vocab(path, texts, pieces=None, omit=()):
    """Write a vocabulary file for `texts` -> {token: id}.
    Every word of basic_tokens(text) gets a line of its own, except: a word in `pieces` ({"playing": ("play", "##ing")}) gets
    lines for its pieces only, a word in `omit` none at all.  Layout: [PAD] on line 0 (the tables' padding is 0 everywhere in
    the project), then fillers, [UNK] on line 7, [CLS] on 11, [SEP] on 13, [MASK] on 14, and from line 17 on a token on every
    THIRD line with two "[unusedN]" fillers between - no id is dense, none of the specials sits where a five-entry tokenizer
    puts it (0 .. 4 in the order PAD, UNK, CLS, SEP, MASK)."""
    pieces = pieces or {}
    want = []
    for text in texts:
        for w in basic_tokens(text):
            for t in pieces.get(w, () if w in omit else (w,)):
                if t not in want:
                    want.append(t)
    fixed = {0: PAD, 7: UNK, 11: CLS, 13: SEP, 14: MASK}
    lines, n_fill = [], 0
    want = sorted(want)
    while want or len(lines) <= max(fixed):
        i = len(lines)
        if i in fixed:
            lines.append(fixed[i])
        elif want and i >= 17 and (i - 17) % 3 == 0:
            lines.append(want.pop(0))
        else:
            lines.append("[unused%d]" % n_fill)
            n_fill += 1
    with open(path, "w", encoding="utf-8") as f:
        f.write("\n".join(lines) + "\n")
    return {t: i for i, t in enumerate(lines)}
