"""Float64 restatement of decoupled weight decay and the warmup / decay schedule of the fused update (csrc/optim.hip:
tnr_adamw_step; engine.py: Engine.step(weight_decay=, warmup_steps=, lr_decay_steps=)).  tests/test_adamw_cpu.py ties it to
torch.optim.AdamW + lr_scheduler.LambdaLR; the GPU tests compare the kernels and the engine against it."""
import numpy as np

import heads_ref as R


def schedule(u, W, T):
    """Multiplier of the learning rate at an update that u updates precede: u / W while u < W; then max(0, (T - u) / max(1, T - W))
    if T > 0 (transformers' get_linear_schedule_with_warmup with num_training_steps = T) and 1 if T == 0
    (get_constant_schedule_with_warmup).  W = T = 0: no schedule."""
    if u < W:
        return float(u) / float(W)
    if T > 0:
        return max(0.0, float(T - u) / float(max(1, T - W)))
    return 1.0


def adamw_step(p, g, m, v, vmax, bc_step, lr, mask, wd, b1=0.9, b2=0.999, eps=1e-8, grad_scale=1.0):
    """torch.optim.AdamW's order: p <- p (1 - lr wd) where mask is set, then heads_ref.adam_step (Adam, AMSGrad when vmax is given)
    on the undecayed gradient grad_scale g.  lr: scalar or per element (already scheduled); mask: bool, scalar or per element;
    bc_step: the number of updates taken, this one included.  -> new (p, m, v, vmax)."""
    p = R.f64(p)
    p = np.where(np.broadcast_to(np.asarray(mask, bool), p.shape), p * (1.0 - np.asarray(lr, np.float64) * wd), p)
    return R.adam_step(p, g, m, v, vmax, bc_step, lr, b1, b2, eps, grad_scale)


def decays(name, shape):
    """A parameter decays iff its name ends in .weight, it is 2-D and its name does not contain LayerNorm."""
    return name.endswith(".weight") and len(shape) == 2 and "LayerNorm" not in name


def decay_mask(names, shapes, offsets, n):
    """bool[n] over a flat buffer: True for the elements of the parameters that decay, False for everything else (exempt
    parameters and the gaps between slots).  names / shapes / offsets: the slot table, one entry per parameter of that buffer."""
    mask = np.zeros(n, dtype=bool)
    for name, shp, o in zip(names, shapes, offsets):
        if decays(name, shp):
            k = int(np.prod(shp))
            assert 0 <= o and o + k <= n and not mask[o:o + k].any(), name
            mask[o:o + k] = True
    return mask


def unpack(words, n):
    """uint32 words (element e = bit e & 31 of word e >> 5) -> bool[n]."""
    w = np.ascontiguousarray(np.asarray(words).view(np.uint32))
    return np.unpackbits(w.view(np.uint8), bitorder="little")[:n].astype(bool)


def pack(mask):
    """bool[n] -> uint32 words, the tail of the last word clear."""
    m = np.zeros((len(mask) + 31) // 32 * 32, dtype=bool)
    m[:len(mask)] = mask
    return np.packbits(m, bitorder="little").view(np.uint32).copy()
