"""CPU side of LAMB (--optimizer lamb): tests/lamb_ref.py against a second, per-parameter torch.float64 implementation and against
tests/adamw_ref.py (trust forced to 1, no decay), the chunk table of engine.lamb_chunks on real and synthetic slot tables with
seeded defects, and the flag surface."""
import numpy as np
import pytest
import torch

import adamw_ref as A
import lamb_ref as L

NAMES = [("enc.query.weight", (6, 5)), ("enc.query.bias", (6,)), ("enc.LayerNorm.weight", (5,)), ("head.att_fc2.bias", (1,)),
         ("head.dense.weight", (3, 7)), ("user.pad_doc", (1, 9)), ("zero.weight", (4, 4)), ("still.weight", (2, 3)),
         ("still.bias", (3,))]


def table_with_gaps(names=NAMES, first=3):
    """Slots back to back in pairs, a gap of 1 .. 5 elements behind every second one, nothing 4-aligned on purpose."""
    out, o = [], first
    for i, (name, shp) in enumerate(names):
        k = int(np.prod(shp))
        out.append((name, o, k, shp))
        o += k + (1 + i % 5 if i % 2 else 0)
    return out, o + 7


def torch_lamb(params, grads, state, t, lr, wd, ams, b1=0.9, b2=0.999, eps=1e-8, grad_scale=1.0):
    """Algorithm 2 of the LAMB paper per named parameter, in torch.float64, written apart from lamb_ref: phi = identity, no clamp,
    bias-corrected moments, decay coupled into the update, layer adaptation for 2-D `.weight`s outside LayerNorm only."""
    trusts = {}
    for name, w in params.items():
        g = grads[name] * grad_scale
        st = state[name]
        st["m"].mul_(b1).add_(g, alpha=1.0 - b1)
        st["v"].mul_(b2).addcmul_(g, g, value=1.0 - b2)
        vhat = st["v"]
        if ams:
            torch.maximum(st["vmax"], st["v"], out=st["vmax"])
            vhat = st["vmax"]
        mhat = st["m"] / (1.0 - b1 ** t)
        r = mhat / ((vhat / (1.0 - b2 ** t)).sqrt() + eps)
        adapt = name.endswith(".weight") and w.dim() == 2 and "LayerNorm" not in name
        u = r + wd * w if adapt else r
        ratio = 1.0
        if adapt:
            wn, un = float(torch.linalg.vector_norm(w)), float(torch.linalg.vector_norm(u))
            if wn > 0.0 and un > 0.0:
                ratio = wn / un
        trusts[name] = ratio
        w.sub_(u, alpha=lr * ratio)
    return trusts


@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("ams", [True, False])
def test_lamb_ref_is_the_per_parameter_float64_lamb(ams, wd):
    """Six steps under warmup 2 / decay 5 on a named set with decay-set and exempt tensors, a zero weight matrix (trust 1: it may
    leave zero) and a tensor pair whose gradient and moments are zero (zero update: trust 1, nothing divided; with wd > 0 the
    matrix still has u = wd w and trust 1 / wd).  Bound 1e-12; gap elements keep their bits in every buffer."""
    table, n = table_with_gaps()
    rs = np.random.RandomState(11)
    flat = [rs.standard_normal(n) for _ in range(2)] + [np.abs(rs.standard_normal(n)) * 0.1 for _ in range(2)]
    p, m, v, x = flat[0], flat[1] * 0.1, flat[2], flat[3] + 0.05
    by = {e[0]: e for e in table}
    for name in ("zero.weight",):
        p[by[name][1]:by[name][1] + by[name][2]] = 0.0
    for name in ("still.weight", "still.bias"):
        s = slice(by[name][1], by[name][1] + by[name][2])
        m[s], v[s], x[s] = 0.0, 0.0, 0.0
    view = lambda buf, e: torch.from_numpy(buf[e[1]:e[1] + e[2]].copy()).view(e[3])
    params = {e[0]: view(p, e) for e in table}
    state = {e[0]: {"m": view(m, e), "v": view(v, e), "vmax": view(x, e)} for e in table}
    ref = [p.copy(), m.copy(), v.copy(), x.copy() if ams else None]
    covered = np.zeros(n, bool)
    for _, o, k, _ in table:
        covered[o:o + k] = True
    assert (~covered).sum() > 10
    lr0, W, TD = 3e-2, 2, 5
    for s in range(6):
        g = rs.standard_normal(n) * 10.0 ** rs.randint(-2, 1)
        for name in ("still.weight", "still.bias"):
            g[by[name][1]:by[name][1] + by[name][2]] = 0.0
        lr = lr0 * A.schedule(s, W, TD)
        trusts = torch_lamb(params, {e[0]: view(g, e) for e in table}, state, s + 1, lr, wd, ams, grad_scale=0.5)
        out = L.lamb_step(table, ref[0], g, ref[1], ref[2], ref[3], s + 1, lr, wd, grad_scale=0.5)
        ref, info = list(out[:4]), out[4]
        for e in table:
            for what, a, b in (("p", params[e[0]], ref[0]), ("m", state[e[0]]["m"], ref[1]), ("v", state[e[0]]["v"], ref[2])) + (
                    (("vmax", state[e[0]]["vmax"], ref[3]),) if ams else ()):
                err = float(np.abs(a.numpy().reshape(-1) - b[e[1]:e[1] + e[2]]).max())
                assert err <= 1e-12, (s, e[0], what, err)
            assert abs(trusts[e[0]] - info[e[0]][0]) <= 1e-12 * abs(trusts[e[0]]), (s, e[0])
        for buf, orig in zip(ref, (p, m, v, x)):
            if buf is not None:
                assert (buf[~covered] == orig[~covered]).all()
        assert all(info[k][0] == 1.0 for k in info if not A.decays(k, by[k][3]))
        assert info["still.bias"][2] == 0.0 and info["still.bias"][0] == 1.0
        if wd == 0.0:
            assert info["still.weight"][2] == 0.0 and info["still.weight"][0] == 1.0      # zero update: trust 1, nothing divided
        else:
            assert abs(info["still.weight"][0] - 1.0 / wd) <= 1e-9 / wd                   # u = wd w alone
        if s == 0:
            assert info["zero.weight"][0] == 1.0 and info["zero.weight"][1] == 0.0 and (ref[0] == p).all()     # rate 0
    assert np.isfinite(ref[0]).all()
    z = by["zero.weight"]
    assert np.abs(ref[0][z[1]:z[1] + z[2]]).min() > 0.0                        # the zero tensor left zero
    st = by["still.weight"]
    moved = not (ref[0][st[1]:st[1] + st[2]] == p[st[1]:st[1] + st[2]]).all()
    assert moved == (wd > 0.0)
    assert any(abs(info[k][0] - 1.0) > 0.1 for k in info if A.decays(k, by[k][3]))                            # the ratio shows


@pytest.mark.parametrize("ams", [True, False])
def test_trust_one_without_decay_is_adam(ams):
    """force_trust = 1 and wd = 0: tests/adamw_ref.adamw_step (mask clear) on the tensors' elements, to 1e-15 relative."""
    table, n = table_with_gaps()
    rs = np.random.RandomState(3)
    p, g, m = rs.standard_normal(n), rs.standard_normal(n) * 0.1, rs.standard_normal(n) * 0.1
    v, x = np.abs(rs.standard_normal(n)) * 0.1, np.abs(rs.standard_normal(n)) * 0.1 + 0.05
    got = L.lamb_step(table, p, g, m, v, x if ams else None, 4, 1e-2, 0.0, grad_scale=0.5, force_trust=1.0)
    want = A.adamw_step(p, g, m, v, x if ams else None, 4, 1e-2, False, 0.0, grad_scale=0.5)
    covered = np.zeros(n, bool)
    for _, o, k, _ in table:
        covered[o:o + k] = True
    for a, b, orig in zip(got[:4], want, (p, m, v, x)):
        if b is not None:
            assert np.allclose(a[covered], b[covered], rtol=1e-15, atol=1e-18) and (a[~covered] == orig[~covered]).all()
    # ... and with the ratio on, the adapted tensors go elsewhere
    free = L.lamb_step(table, p, g, m, v, x if ams else None, 4, 1e-2, 0.0, grad_scale=0.5)
    assert np.abs(free[0] - got[0]).max() > 1e-4


def test_trust_bound_is_below_the_optimiser_bound():
    assert L.ADD_PATH == 17 and L.ELEM_ROUNDINGS == 13
    assert abs(L.trust_rtol(1.0) - 31 * L.U) < 1e-12 and L.trust_rtol(1.0) < 2e-6 and L.trust_rtol(3.0) < 1e-5
    assert L.norm_rtol(1.0, of_u=False) < L.norm_rtol(1.0) < L.trust_rtol(1.0) + L.U


def _check(table, n, names, chunks, tensors):
    L.check_chunks(table, n, chunks, tensors, names)


def _rejected(table, n, names, chunks, tensors=None):
    with pytest.raises(AssertionError):
        L.check_chunks(table, n, chunks, tensors, names)


def _seeded_defects(table, n, names, chunks):
    """A dropped element, a chunk crossing into the next tensor, a covered gap, an oversized chunk, a wrong tensor id, a wrong flag,
    a doubled chunk: each must be rejected."""
    c = chunks.copy()
    c[0, 1] -= 1
    if c[0, 1] == 0:
        c = c[1:]
    _rejected(table, n, names, c)                                           # the last element of the first chunk is dropped
    by = {e[0]: e for e in table}
    ends = {by[nm][1] + by[nm][2]: nm for nm in names}
    starts = {by[nm][1] for nm in names}
    last_of = [j for j in range(len(chunks)) if chunks[j, 0] + chunks[j, 1] in ends]
    into_next = [j for j in last_of if chunks[j, 0] + chunks[j, 1] in starts and chunks[j, 1] < L.CHUNK]
    into_gap = [j for j in last_of if chunks[j, 0] + chunks[j, 1] not in starts and chunks[j, 0] + chunks[j, 1] < n and chunks[j, 1] < L.CHUNK]
    assert into_next and into_gap, "the table has no back-to-back pair or no gap"
    for j in (into_next[0], into_gap[0]):
        c = chunks.copy()
        c[j, 1] += 1
        _rejected(table, n, names, c)
    c = chunks.copy()
    c[0, 2] = (c[0, 2] + 1) % len(names)
    _rejected(table, n, names, c)
    c = chunks.copy()
    c[0, 3] ^= 1
    _rejected(table, n, names, c)
    _rejected(table, n, names, np.concatenate([chunks, chunks[:1]]))
    big = [j for j in range(len(chunks) - 1) if chunks[j, 2] == chunks[j + 1, 2] and chunks[j, 1] == L.CHUNK]
    if big:                                                                 # two chunks of a tensor merged: 4096 + more
        j = big[0]
        c = np.delete(chunks, j + 1, axis=0)
        c[j, 1] += chunks[j + 1, 1]
        _rejected(table, n, names, c)


def test_chunk_table_of_a_synthetic_slot_table():
    import engine as E
    sizes = [1, 3, 4, 5, 255, 4095, 4096, 4097, 2 * 4096 + 1, 7, 4096, 1]
    names = [("t%d.%s" % (i, "weight" if i % 3 != 1 else "bias"), (k, 1) if i % 3 != 1 else (k,)) for i, k in enumerate(sizes)]
    table, n = table_with_gaps(names, first=1)
    slot = {name: (True, o, k, shp) for name, o, k, shp in table}
    slot["frozen.weight"] = (False, 0, 100, (10, 10))                       # frozen tensors live in another buffer: no chunk
    got_names, chunks, tensors = E.lamb_chunks(slot, n)
    assert chunks.dtype == np.int32 and chunks.shape[1] == 4 and tensors.dtype == np.int32 and tensors.shape == (len(sizes), 4)
    assert got_names == [e[0] for e in sorted(table, key=lambda e: e[1])]
    _check(table, n, got_names, chunks, tensors)
    assert chunks[:, 1].max() == 4096 and chunks[:, 1].min() == 1
    assert {int(f) % 4 for f in chunks[:, 0]} == {0, 1, 2, 3}               # chunks start at every offset modulo 4
    inner = [j for j in range(1, len(chunks)) if chunks[j, 2] == chunks[j - 1, 2]]
    assert inner and all(chunks[j, 0] % 4096 == 0 for j in inner)           # inside a tensor chunks start 16-byte aligned
    _seeded_defects(table, n, got_names, chunks)
    t2 = tensors.copy()
    t2[3, 1] += 1
    _rejected(table, n, got_names, chunks, t2)
    again = E.lamb_chunks(slot, n)
    assert again[0] == got_names and (again[1] == chunks).all() and (again[2] == tensors).all()     # a pure function


@pytest.mark.parametrize("train_embeddings", [False, True])
def test_chunk_table_of_the_test_engines_slot_table(train_embeddings):
    """The 2-layer, 2-teacher engine of the GPU tests: exact cover of every trainable tensor, the gaps between groups and the
    reserved rows behind att_fc1 uncovered, the one-element att_fc2.bias a chunk of its own, one table for engines that share."""
    import engine as E
    cfg = E.EngineConfig(n_layers=2, trainable_layers=(0, 1), num_teachers=2, train_embeddings=train_embeddings)
    eng = E.Engine(cfg, device="cpu", max_batch=1)
    assert eng._lamb_state is None and eng.trust_ratios() is None
    table = L.slots(eng.slot)
    names, chunks, tensors = E.lamb_chunks(eng.slot, eng.n_train)
    _check(table, eng.n_train, names, chunks, tensors)
    assert len(names) == len(table) and sum(e[2] for e in table) == int(chunks[:, 1].sum()) < eng.n_train
    fc1 = E.PFX + "attn.att_fc1.weight"
    end = eng.slot[fc1][1] + eng.slot[fc1][2]
    nxt = min(e[1] for e in table if e[1] >= end)
    assert nxt - end >= 64                                                   # the reserved rows: covered by no chunk (checked above)
    ue = "student.user_encoder."
    o = eng.off(ue + "attn.att_fc2.bias")
    one = [c for c in chunks.tolist() if c[0] == o]
    assert one == [[o, 1, names.index(ue + "attn.att_fc2.bias"), 0]]
    emb = E.BERT + "embeddings.word_embeddings.weight"
    assert (emb in names) == train_embeddings
    assert not any(k.startswith("teachers.") for k in names)
    adapted = [names[t] for t in range(len(names)) if tensors[t, 2]]
    assert adapted == [k for k in names if A.decays(k, eng.slot[k][3])] and 0 < len(adapted) < len(names)
    _seeded_defects(table, eng.n_train, names, chunks)
    second = E.Engine(cfg, device="cpu", max_batch=1, share=eng)
    assert second._clip_owner is eng and second._lamb_state is None and eng._lamb_state is None      # nothing before a step asks
    # the rate ranges of Engine.step start where a chunk starts
    firsts = set(int(f) for f in chunks[:, 0])
    head0 = eng.off(fc1)
    e = eng.off(E.PFX + "dense.bias") + eng.slot[E.PFX + "dense.bias"][2]
    rest0 = min((e + 63) // 64 * 64, eng.n_train)
    assert head0 in firsts and (rest0 in firsts or rest0 == eng.n_train)


def test_flags():
    import parameters
    import post_train_kd
    import run
    from model_bert import TnrAdam
    a = parameters.parse_args([])
    # an adam run's checkpoint keeps the flags it always held: the key is recorded when it is not the default
    assert a.optimizer == "adam" and "optimizer" not in run._train_flags(a, 2)
    b = parameters.parse_args(["--optimizer", "lamb", "--weight_decay", "0.01"])
    assert b.optimizer == "lamb" and run._train_flags(b, 8)["optimizer"] == "lamb" and run._train_flags(b, 8)["world"] == 8
    for mod in (parameters, post_train_kd):
        with pytest.raises(SystemExit):
            mod.parse_args(["--optimizer", "bogus"])
    assert post_train_kd.parse_args([]).optimizer == "adam" and post_train_kd.parse_args(["--optimizer", "lamb"]).optimizer == "lamb"
    helps = {f[0]: f[3].get("help", "") for f in parameters._FLAGS if len(f) > 3}
    assert "coupled" in helps["weight_decay"].lower() and "coupled" in helps["optimizer"].lower()
    assert TnrAdam(None, 1e-4).optimizer == "adam" and TnrAdam(None, 1e-4, optimizer="lamb").optimizer == "lamb"
    with pytest.raises(ValueError):
        TnrAdam(None, 1e-4, optimizer="lars")


def test_tnradam_hands_lamb_to_the_engine_only_when_on():
    from model_bert import TnrAdam
    seen = []

    class Eng:
        def step(self, lr, **kw):
            seen.append(kw)

    class Model:
        engine = Eng()
    TnrAdam(Model(), 1e-4).step()
    TnrAdam(Model(), 1e-4, optimizer="lamb", weight_decay=0.01).step()
    assert "lamb" not in seen[0] and seen[1]["lamb"] is True and seen[1]["weight_decay"] == 0.01
