"""Float64 restatement of LAMB (You et al., "Large Batch Optimization for Deep Learning", Algorithm 2) as the fused step states it
(include/tnr_hip.h: tnr_lamb_norms / _commit / _step; engine.py: Engine.step(lamb=True)), the checker of the chunk table
(engine.lamb_chunks) and the derived error bound of the trust ratios.  tests/test_lamb_cpu.py ties the restatement to a second,
per-parameter torch.float64 implementation and to tests/adamw_ref.py; the GPU tests compare the kernels and the engine against it.

The restatement walks the slot table tensor by tensor and knows nothing of chunks.  A slot table here is a list of
(name, offset, numel, shape), one entry per trainable tensor of one flat buffer (`slots(engine.slot)` makes it).

The hyperparameters reach the kernels as C floats, so the reference takes them through f32(): the kernels' inputs are the rounded
values (1 - b for b in [0.5, 1] is then exact in fp32, Sterbenz), and the bounds below count the roundings of the arithmetic alone.
"""
import numpy as np

import adamw_ref as A

U = 2.0 ** -24                      # unit roundoff of fp32
CHUNK = 4096


def f32(x):
    """A host double as the C float the entry points receive, back in float64."""
    return float(np.float32(x))


def slots(engine_slot):
    """engine.slot -> [(name, offset, numel, shape)] of the trainable tensors, in the table's own order."""
    return [(k, int(o), int(n), tuple(shp)) for k, (tr, o, n, shp) in engine_slot.items() if tr]


def lamb_step(table, p, g, m, v, vmax, bc_step, lr, wd, b1=0.9, b2=0.999, eps=1e-8, grad_scale=1.0, force_trust=None):
    """One LAMB update over the flat float64 buffers p, g, m, v (vmax: AMSGrad, None: Adam); -> (p, m, v, vmax, info).
    Per tensor of `table`:  g' = grad_scale g;  m = b1 m + (1 - b1) g';  v = b2 v + (1 - b2) g'^2;  vhat = max(vmax, v) or v;
    r = (m / (1 - b1^t)) / (sqrt(vhat) / sqrt(1 - b2^t) + eps);  u = r + wd w if A.decays(name, shape) else r;
    trust = ||w|| / ||u|| if the tensor decays (is adapted) and both norms are non-zero, else 1;  w <- w - lr trust u.
    lr: scalar or per element (already scheduled), bc_step = t: the updates taken, this one included.  Elements outside every
    tensor keep their values in all buffers.  info[name] = (trust, ||w||, ||u||, kappa) with kappa = sqrt(sum a^2 / sum u^2),
    a = the sum of the magnitudes of u's terms (the condition number trust_rtol wants); force_trust: that value instead of the
    ratio for every adapted tensor."""
    p, g, m, v = (np.array(x, np.float64) for x in (p, g, m, v))
    vmax = None if vmax is None else np.array(vmax, np.float64)
    lr = np.broadcast_to(np.asarray(lr, np.float64), p.shape)
    c1, c2 = 1.0 - b1 ** bc_step, 1.0 - b2 ** bc_step
    info = {}
    for name, o, n, shp in table:
        s = slice(o, o + n)
        w, gs = p[s].copy(), g[s] * grad_scale
        m2 = m[s] * b1 + (1.0 - b1) * gs
        v2 = v[s] * b2 + (1.0 - b2) * gs * gs
        vh = v2 if vmax is None else np.maximum(vmax[s], v2)
        den = np.sqrt(vh) / np.sqrt(c2) + eps
        r = (m2 / c1) / den
        adapted = A.decays(name, shp)
        u = r + wd * w if adapted else r
        mag = (np.abs(m[s] * b1) + np.abs((1.0 - b1) * gs)) / c1 / den + (np.abs(wd * w) if adapted else 0.0)
        wn, un = float(np.sqrt((w * w).sum())), float(np.sqrt((u * u).sum()))
        trust = 1.0
        if adapted:
            trust = (wn / un if (wn != 0.0 and un != 0.0) else 1.0) if force_trust is None else float(force_trust)
        kappa = float(np.sqrt((mag * mag).sum()) / un) if un != 0.0 else 1.0
        info[name] = (trust, wn, un, kappa)
        p[s] = w - lr[s] * trust * u
        m[s], v[s] = m2, v2
        if vmax is not None:
            vmax[s] = vh
    return p, m, v, vmax, info


# ---- the error bound of trust ------------------------------------------------------------------------------------------------
# trust = sqrt(Sw / Su), Sw = sum w^2 and Su = sum u^2 over the tensor.
# Summation (csrc/lamb.hip: lamb_norm_kernel, the shape of grad_sumsq_kernel).  All terms are non-negative, so the relative error
# of the fp32 sum is at most (longest addition path) x 2^-24 to first order.  Per chunk of <= 4096 elements a lane feeds component
# 0 of its four running sums with at most one head scalar, one tail scalar and four 16-byte groups (6 fmas; the square is exact
# inside the fma); then (s0 + s1) + (s2 + s3) (2), the butterfly over 64 lanes (6), four waves in wave order (3): 17 additions.
# The chunk partials are summed in double (2^-53 per addition: nothing).
ADD_PATH = 17
# Per element of u (lamb_elem): g' = g gscale (1 rounding); (1 - b1) g' (1) and the fma that forms m (1): 3 on m, relative to
# |b1 m| + |(1 - b1) g'| (the two may cancel); v: g' (1), (1 - b2) g' (1), x g' (1 + g''s 1), fma (1): 5, relative (non-negative
# terms); sqrt halves that and rounds (3.5); the fma with the rounded 1 / sqrt(c2) and eps (non-negative terms): + 2 = 5.5 on
# the denominator; the divide (1), the rounded 1 / c1 (1) and its product (1): r carries 3 + 5.5 + 3 = 11.5; the fma with wd w:
# + 1.  Rounded up: 13 x 2^-24 of a = the sum of the magnitudes of u's terms.
ELEM_ROUNDINGS = 13


def trust_rtol(kappa=1.0):
    """|trust - ref| <= trust_rtol(kappa) |ref|.  With u_hat = u + e, |e| <= eps a, eps = ELEM_ROUNDINGS x 2^-24:
    |sum u_hat^2 - sum u^2| <= 2 eps sqrt(sum u^2) sqrt(sum a^2) + eps^2 sum a^2, i.e. 2 eps kappa + (eps kappa)^2 of Su; both sums
    carry ADD_PATH x 2^-24 of summation error; the square root halves the total; the fp32 store of trust adds 2^-24.  kappa = 1
    when no term of u cancels.  Comes out at 31 x 2^-24 = 1.85e-6 for kappa = 1, below the 1e-5 the optimiser tests use for
    parameters."""
    e = ELEM_ROUNDINGS * U * float(kappa)
    return 0.5 * (2.0 * ADD_PATH * U + 2.0 * e + e * e) + U


def norm_rtol(kappa=1.0, of_u=True):
    """The same for the two norms trust came from (fp32 stores of sqrt(S))."""
    e = ELEM_ROUNDINGS * U * float(kappa) if of_u else 0.0
    return 0.5 * (ADD_PATH * U + 2.0 * e + e * e) + U


# ---- the chunk table ---------------------------------------------------------------------------------------------------------
def check_chunks(table, n, chunks, tensors=None, names=None):
    """Raise AssertionError unless `chunks` (rows: first, count, tensor id, flags) is a valid map of `table` over a flat buffer of n
    elements: every element of every tensor in exactly one chunk, nothing else covered (gaps, reserved rows), no chunk across a
    tensor's end, 1 <= count <= 4096, the tensor id that of the tensor the chunk lies in (ids index `names`, default: the table
    sorted by offset), flag bit 0 == A.decays, a tensor's chunks consecutive; `tensors` (rows: first chunk, number of chunks,
    adapted, 0), when given, must say the same."""
    order = sorted(table, key=lambda e: e[1])
    if names is None:
        names = [e[0] for e in order]
    by_name = {e[0]: e for e in table}
    assert len(names) == len(table) and set(names) == set(by_name), "tensor ids do not name the table's tensors"
    chunks = np.asarray(chunks).reshape(-1, 4)
    owner = np.full(n, -1, dtype=np.int64)
    for t, name in enumerate(names):
        _, o, k, _ = by_name[name]
        assert 0 <= o and o + k <= n and (owner[o:o + k] == -1).all(), "slot table overlaps at %s" % name
        owner[o:o + k] = t
    cover = np.zeros(n, dtype=np.int64)
    runs = {}
    for j, (first, count, t, flags) in enumerate(chunks.tolist()):
        assert 1 <= count <= CHUNK, "chunk %d: count %d" % (j, count)
        assert 0 <= first and first + count <= n, "chunk %d outside the buffer" % j
        assert 0 <= t < len(names), "chunk %d: tensor id %d" % (j, t)
        name, o, k, shp = by_name[names[t]]
        assert o <= first and first + count <= o + k, "chunk %d crosses the bounds of %s (or covers a gap)" % (j, name)
        assert (owner[first:first + count] == t).all(), "chunk %d covers elements that are not %s's" % (j, name)
        assert (flags & 1) == int(A.decays(name, shp)), "chunk %d: flag of %s" % (j, name)
        cover[first:first + count] += 1
        runs.setdefault(t, []).append(j)
    assert (cover[owner >= 0] == 1).all(), "an element of a tensor is covered %s" % (
        "twice" if (cover[owner >= 0] > 1).any() else "by no chunk")
    assert (cover[owner < 0] == 0).all(), "a gap element is covered"
    for t, js in runs.items():
        assert js == list(range(js[0], js[0] + len(js))), "the chunks of %s are not consecutive" % names[t]
    assert set(runs) == set(range(len(names))), "a tensor has no chunk"
    if tensors is not None:
        tensors = np.asarray(tensors).reshape(-1, 4)
        assert len(tensors) == len(names)
        for t, (fc, nc, ad, _) in enumerate(tensors.tolist()):
            assert (fc, nc) == (runs[t][0], len(runs[t])), "tensor table entry %d" % t
            assert ad == int(A.decays(names[t], by_name[names[t]][3])), "adapted flag of %s" % names[t]
