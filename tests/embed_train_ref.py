"""Shared by tests/test_embed_train_cpu.py and tests/test_embed_train_gpu.py: the gradients of a training step with the embedding
block trainable, from oracle/torch_port.model_forward + torch autograd (fp32, CPU).  The port indexes word[ids] without a padding
row, so row 0 of its word-table gradient is zeroed here: nn.Embedding(padding_idx=0) of tnlrv3/modeling.py:138 never gives that
row a gradient (tests/golden/plmnr_embed_0.npz pins it)."""
import numpy as np
import torch

from oracle import torch_port as TP

EMB = TP.BERT + "embeddings."
EMB_KEYS = [EMB + k for k in ("word_embeddings.weight", "position_embeddings.weight", "token_type_embeddings.weight",
                              "LayerNorm.weight", "LayerNorm.bias")]
WORD = EMB_KEYS[0]


def port_grads(P, cfg, hist, mask, cand, label, th=(), tc=()):
    """-> (total loss, score (B, C), {key: gradient}) over the reference's trainable set plus the five embedding parameters."""
    Pt = TP.make_params(P, cfg["trainable_layers"])
    for k in EMB_KEYS:
        Pt[k].requires_grad_(True)
    t = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x)).to(dt)
    out = TP.model_forward(Pt, cfg, t(hist, torch.int64), t(mask, torch.float32), t(cand, torch.int64), t(label, torch.int64),
                           [t(x, torch.float32) for x in th], [t(x, torch.float32) for x in tc])
    out[0].backward()
    G = {k: v.grad.numpy() for k, v in Pt.items() if v.requires_grad and v.grad is not None}
    G[WORD] = G[WORD].copy()
    G[WORD][0] = 0.0
    return float(out[0].detach()), out[4].detach().numpy(), G


def rel_l2(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.sqrt(((got - ref) ** 2).sum()) / (np.sqrt((ref ** 2).sum()) + 1e-30))
