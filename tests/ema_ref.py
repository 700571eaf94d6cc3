"""Float64 restatement of the exponential moving average of the weights in the fused update (csrc/optim.hip: tnr_adamw_step_ema;
engine.py: Engine.step(ema_decay=, ema_warmup=)).  tests/test_ema_cpu.py ties it to torch.optim.swa_utils.AveragedModel with
get_ema_multi_avg_fn; the GPU tests compare the kernel and the engine against it."""
import numpy as np

import adamw_ref as A
import heads_ref as R


def decay_at(u, decay, warmup):
    """Decay of the average at an update that u updates precede: `decay`, or with warmup min(decay, (1 + u) / (10 + u)) -
    TensorFlow's ExponentialMovingAverage(decay, num_updates=u)."""
    if warmup:
        return min(float(decay), (1.0 + float(u)) / (10.0 + float(u)))
    return float(decay)


def ema_step(e, p_new, w):
    """e + w (p_new - e), w = 1 - decay: decay e + (1 - decay) p_new."""
    e = R.f64(e)
    return e + np.asarray(w, np.float64) * (R.f64(p_new) - e)


def adamw_ema_step(p, g, m, v, vmax, e, bc_step, lr, mask, wd, w, b1=0.9, b2=0.999, eps=1e-8, grad_scale=1.0, skipped=False):
    """adamw_ref.adamw_step, then ema_step on the new parameters.  skipped (the fp16 guard found inf / nan in the gradient):
    everything comes back untouched, the average included.  -> new (p, m, v, vmax, e)."""
    if skipped:
        return R.f64(p), R.f64(m), R.f64(v), (None if vmax is None else R.f64(vmax)), R.f64(e)
    p, m, v, vmax = A.adamw_step(p, g, m, v, vmax, bc_step, lr, mask, wd, b1, b2, eps, grad_scale)
    return p, m, v, vmax, ema_step(e, p, w)
