"""Generate tests/golden/plmnr_embed_0.npz by executing the REFERENCE's own Python: golden_plmnr of make_golden.py (PLM-NR's
ModelBert, freeze policy and two-learning-rate AMSGrad of PLM-NR/run.py:84-106, two optimiser steps) with the parameters of
bert.embeddings left requires_grad=True in addition to the listed layers -- what --train_embeddings computes.

Run once where the reference is present:  python tests/golden/make_golden_embed.py
Data only: inputs, losses, scores, gradient norms / samples, and for the word table whole gradient rows of row 0 (padding_idx of
tnlrv3/modeling.py:138: exactly zero), of the most frequent id, of two ids that occur once and of two ids that never occur, plus
the list of ids with a non-zero row; parameter samples (and those rows) after the second step."""
import os

import numpy as np
import torch

import make_golden as G          # sets sys.path, imports ref_shim and hashinit; its own fixtures are untouched

ref_shim, hashinit = G.ref_shim, G.hashinit
EMB = "news_encoder.bert_model.bert.embeddings."
WORD = EMB + "word_embeddings.weight"


def golden_plmnr_embed(out_name="plmnr_embed_0.npz", seed=41, nl=2, trainable=(0, 1)):
    R = ref_shim.load_reference("PLM-NR")
    B = 2
    cfg_json = dict(ref_shim.BASE_CFG, num_hidden_layers=nl)
    a = ref_shim.make_args(config_name=ref_shim.write_config(cfg_json), num_hidden_layers=nl, batch_size=B)
    model = R.model_bert.ModelBert(a)
    with torch.no_grad():
        for k, v in model.state_dict().items():
            v.copy_(torch.from_numpy(hashinit.init_tensor(seed, "student." + k, tuple(v.shape))))
    bm = model.news_encoder.bert_model
    for p in bm.parameters():
        p.requires_grad = False
    for i, layer in enumerate(bm.bert.encoder.layer):
        if i in trainable:
            for p in layer.parameters():
                p.requires_grad = True
    for p in bm.bert.embeddings.parameters():
        p.requires_grad = True
    L = a.num_words_title
    inp = G.make_inputs(seed, B, a.user_log_length, a.npratio + 1, L, cfg_json["vocab_size"], 0, a.news_dim)
    hist, mask, cand, label = inp[:4]
    tt = lambda x: torch.from_numpy(np.ascontiguousarray(x))
    named = dict(model.named_parameters())
    bert = [p for n, p in named.items() if ".bert_model." in n]
    rest = [p for n, p in named.items() if ".bert_model." not in n]
    lr_bert, lr = 1e-5, 1e-4
    opt = torch.optim.Adam([{"params": bert, "lr": lr_bert}, {"params": rest, "lr": lr}], amsgrad=True)
    rec = dict(in_hist=hist, in_mask=mask, in_cand=cand, in_label=label, lrs=np.array([lr_bert, lr]),
               meta=np.array([seed, B, 0, a.user_log_length, a.npratio + 1, L, a.news_dim,
                              cfg_json["num_attention_heads"], nl]), trainable=np.array(trainable))
    # the word rows that are stored whole
    ids = np.concatenate([hist[..., :L].reshape(-1), cand[..., :L].reshape(-1)])
    cnt = np.bincount(ids, minlength=cfg_json["vocab_size"])
    seen = np.nonzero(cnt[1:])[0] + 1
    once = np.nonzero(cnt == 1)[0][:2]
    never = np.nonzero(cnt == 0)[0][[0, -1]]
    rows = np.concatenate([[0, seen[np.argmax(cnt[seen])]], once, never]).astype(np.int64)
    rec["word_rows"], rec["word_row_counts"] = rows, cnt[rows]
    names = []
    for step in range(2):
        opt.zero_grad()
        loss, score = model(tt(hist), tt(mask), tt(cand), tt(label))
        loss.backward()
        rec["loss%d" % step] = loss.item()
        rec["score%d" % step] = score.detach().numpy()
        if step == 0:
            for n, p in named.items():
                if p.grad is None:
                    continue
                g = p.grad.numpy()
                names.append(n)
                rec["gnorm." + n] = np.float64(np.sqrt((g.astype(np.float64) ** 2).sum()))
                idx, val = G.grad_samples(seed, n, g)
                rec["gidx." + n], rec["gval." + n] = idx, val
            gw = named[WORD].grad.numpy()
            rec["word_grad_rows"] = gw[rows].copy()
            rec["word_nonzero_ids"] = np.nonzero(np.abs(gw).max(1))[0].astype(np.int64)
            for n in ("position_embeddings.weight", "token_type_embeddings.weight", "LayerNorm.weight", "LayerNorm.bias"):
                g = named[EMB + n].grad.numpy()
                rec["grad." + EMB + n] = g[:L + 2].copy() if g.ndim == 2 else g.copy()      # position rows >= L: zero
        opt.step()
    rec["grad_names"] = np.array(names)
    for n in ("news_encoder.dense.weight", "news_encoder.bert_model.bert.encoder.layer.%d.output.dense.weight" % max(trainable),
              "user_encoder.attn.att_fc1.weight", EMB + "LayerNorm.weight", EMB + "position_embeddings.weight"):
        w = named[n].detach().numpy()
        if n.endswith("position_embeddings.weight"):
            w = w[:L]                                                # the rows that move
        idx, val = G.grad_samples(seed, "w." + n, w)
        rec["widx." + n], rec["wval." + n] = idx, val                # parameter samples after the two steps
    rec["word_rows_after"] = named[WORD].detach().numpy()[rows].copy()
    np.savez_compressed(os.path.join(G.HERE, out_name), **rec)
    print(out_name, rec["loss0"], rec["loss1"], "rows", rows, cnt[rows], "non-zero rows", len(rec["word_nonzero_ids"]))


if __name__ == "__main__":
    golden_plmnr_embed()
