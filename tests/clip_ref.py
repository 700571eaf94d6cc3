"""float64 numpy restatement of global-norm gradient clipping (csrc/optim.hip: grad_sumsq_kernel, grad_clip_commit_kernel,
amsgrad_kernel<., CLIP>; engine.Engine.step(max_grad_norm=...)) and the error bound of the kernels' sum of squares.
tests/test_grad_clip_cpu.py ties the formula to torch.nn.utils.clip_grad_norm_.

  total_norm = grad_scale * sqrt(sum g^2) ; coef = min(1, max_norm / (total_norm + 1e-6)) ; the optimiser sees coef * grad_scale * g.

Bound of the sum of squares: relative (c + 1) * 2^-23, every term being positive.  c = sumsq_depth(n) is the longest chain of
fp32 additions one term passes through in grad_sumsq_kernel as written: a lane folds component r of its 16-byte reads into running
sum r, four additions per trip of the grid-stride loop (trips = ceil(blocks / grid), blocks = ceil(n / 4096), grid = min(blocks,
2048)); then (s0 + s1) + (s2 + s3): 2; the wave butterfly: 6; the four waves in wave order: 3.  The + 1 is the square itself (the
kernel forms it inside an fma, so it is slack).  The sum over the partials is in double and adds nothing."""
import numpy as np

U23 = 2.0 ** -23
BLOCK, GRID_CAP = 4096, 2048


def f64(x):
    return np.asarray(x, np.float64)


def sumsq_parts(n):
    """tnr_grad_sumsq_parts: workgroups (= partial sums) of a scan over n elements."""
    return max(1, min((n + BLOCK - 1) // BLOCK, GRID_CAP))


def sumsq_depth(n):
    blocks = (n + BLOCK - 1) // BLOCK
    trips = (blocks + sumsq_parts(n) - 1) // sumsq_parts(n)
    return 4 * trips + 2 + 6 + 3


def sumsq_rtol(ns):
    """Relative bound of the sum of squares over slices of ns elements each (one commit over all their partials)."""
    return (max(sumsq_depth(n) for n in ns) + 1) * U23


def clip(grads, max_norm, grad_scale=1.0):
    """grads: arrays (the parameters' gradients before grad_scale).  -> (total_norm, coef), float64; inf / nan as numpy gives them."""
    with np.errstate(over="ignore", invalid="ignore"):
        total = grad_scale * np.sqrt(sum(float((f64(g) ** 2).sum()) for g in grads))
        c = max_norm / (total + 1e-6)
    return total, (1.0 if c > 1.0 else c)
