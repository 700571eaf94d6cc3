"""Generate tests/golden/title_vocab.json from the REFERENCE's vocabulary file and tests/golden/datapath.npz.

Run once where the reference is checked out (read-only, absent on the GPU box):
    python tests/golden/make_title_vocab.py <reference>/Tiny-NewsRec/tnlrv3/tokenizer/tnlrv3-base-uncased-vocab.txt
Only names are written: the (token, id) pairs of the ids that datapath.npz: news_combined holds (the table the reference's
preprocess.py made of tests/golden/data/news.tsv), the ids of the five special tokens and the number of lines of the file.
tests/test_tokenize_cpu.py writes a vocabulary file of that many lines from them (fillers elsewhere) and never reads the
reference.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SPECIALS = ("[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]")


def main(vocab_path):
    with open(vocab_path, encoding="utf-8") as f:
        tokens = [ln.rstrip("\n") for ln in f]
    comb = np.load(os.path.join(HERE, "datapath.npz"))["news_combined"]
    width = comb.shape[1] // 2
    used = sorted(int(i) for i in np.unique(comb[:, :width]))
    out = dict(size=len(tokens), specials={s: tokens.index(s) for s in SPECIALS}, tokens=[[tokens[i], i] for i in used])
    with open(os.path.join(HERE, "title_vocab.json"), "w") as f:
        json.dump(out, f, indent=1, ensure_ascii=True)
        f.write("\n")
    print("%d lines, %d ids used by news_combined: %s" % (len(tokens), len(used), out["tokens"]))


if __name__ == "__main__":
    main(sys.argv[1])
