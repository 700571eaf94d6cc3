"""GPU: the two caches an Engine makes for a resident token table - the frozen-layer cache (build_frozen_cache / encode) and the
RoBERTa position ids (_pos_ids, pos_pad_id set) - serve a table only as long as it is THAT table with THOSE contents.

Both were keyed by the table's address (and shape) alone.  A table refreshed in place (a loader that rewrites its resident table),
or a table freed and another allocated where it lay (a validation table made each round), silently got the old table's hidden
states or position ids; a view with fewer rows took the whole table's frozen cache.  Engine._table_key now holds the address, shape,
dtype and torch's version counter, and the entry keeps the table tensor, so its address cannot be handed out again.

Every case runs on tests/history_ref.py's model (layer 0 frozen: the cache applies) and compares a whole training step, bit for
bit, with a fresh engine that never had a cache and is fed the table the step is meant to see: torch.equal on losses, scores, S and
flat_g.  No tolerance: the cache is bit-identical to recomputing (rows are processed independently)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import engine as E                                               # noqa: E402
import history_ref as HR                                         # noqa: E402

DEV = "cuda:0"
WHAT = ("losses", "score", "S", "flat_g")
POS_PAD = 1
_DEV = {}


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _tables(roberta):
    """-> (A, A2) numpy (401, 2 L) int32: history_ref's table and the same rows in reverse order behind the pad row (another title,
    of another length, in every row).  roberta: padding positions hold the id POS_PAD instead of 0, as RoBERTa's vocabulary has it."""
    A = HR.news().copy()
    if roberta:
        ids, mask = A[:, :HR.L], A[:, HR.L:]
        assert not (ids == POS_PAD).any()
        ids[mask == 0] = POS_PAD
    A2 = A.copy()
    A2[1:] = A[1:][::-1]
    assert A2.shape == A.shape and not np.array_equal(A, A2)
    return A, A2


def _engine(dtype, B, **more):
    eng = E.Engine(E.EngineConfig(**HR.engine_kwargs(), **more), DEV, max_batch=B, dtype=dtype)
    if "P" not in _DEV:
        _DEV.update(P={k: _t(v) for k, v in HR.weights().items()}, tables=_t(HR.teachers()))
    eng.load_state_dict(_DEV["P"])
    return eng


def _step(eng, table, fid):
    """forward_indexed + backward over `table` -> clones of what is compared."""
    if fid not in _DEV:
        _DEV[fid] = tuple(_t(x) for x in HR.feed(fid))
    h, m, c, y = _DEV[fid]
    losses, score = eng.forward_indexed(table, h, m, c, y, _DEV["tables"])
    eng.backward()
    B, _, Rt = eng.cur
    return dict(losses=losses.clone(), score=score.clone(), S=eng.S[:Rt].clone(), flat_g=eng.flat_g.clone())


def _same(a, b):
    return all(torch.equal(a[k], b[k]) for k in WHAT)


def _count_embed(eng):
    """-> a list that grows by one with every embedding launch of `eng` (a pass that does not take the frozen cache)."""
    calls, real = [], eng._embed_fwd

    def counted(*a):
        calls.append(a[1])
        return real(*a)
    eng._embed_fwd = counted
    return calls


# which cache: (EngineConfig keywords, batch, feed, uses build_frozen_cache).  The position-id cache is for tables of more than
# 4 N_alloc rows: 401 > 4 x 100 at the short batch.
CACHES = {"fcache": (dict(), HR.B_FULL, "full_a", True), "pos_cache": (dict(pos_pad_id=POS_PAD), HR.B_SHORT, "short_a", False)}


def _cached_step(which, dtype, A):
    """An engine that has made its cache for the device table A and run a step over it -> (engine, feed id, fresh-engine maker)."""
    more, B, fid, frozen = CACHES[which]
    eng = _engine(dtype, B, **more)
    if frozen:
        assert eng.build_frozen_cache(A) and eng.fcache is not None
        calls = _count_embed(eng)
        first = _step(eng, A, fid)
        assert not calls                                                          # the step went through the cache
    else:
        assert A.shape[0] > 4 * eng.N_alloc
        first = _step(eng, A, fid)
        c = eng._pos_cache
        assert c is not None and c[0][0] == A.data_ptr() and c[1].shape == (A.shape[0], HR.L)       # the cache was made ...
        assert eng._pos_ids(A) is c[1]                                            # ... and is what the next pass over A gets
    return eng, fid, first, (lambda: _engine(dtype, B, **more))


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("which", list(CACHES))
def test_a_table_rewritten_in_place_is_not_served_the_old_entry(which, dtype):
    """build the cache for A, step; A.copy_(A2) without rebuilding; the next step equals a fresh engine fed A2."""
    a, a2 = _tables(which == "pos_cache")
    if which == "pos_cache":
        assert ((a[:, :HR.L] == POS_PAD) != (a2[:, :HR.L] == POS_PAD)).any(1).sum() > 200          # the pad tokens lie elsewhere
    A, A2 = _t(a), _t(a2)
    eng, fid, first, fresh = _cached_step(which, dtype, A)
    assert _same(first, _step(fresh(), A, fid))                                   # through the cache: what recomputing gives
    ptr = A.data_ptr()
    A.copy_(A2)
    assert A.data_ptr() == ptr
    got = _step(eng, A, fid)
    want = _step(fresh(), A2, fid)
    torch.cuda.synchronize()
    assert not _same(first, want)                                                 # the contents matter
    for k in WHAT:
        assert torch.equal(got[k], want[k]), "%s: %s of the step over the rewritten table differs from a fresh engine's in %d elements " \
            "(equals the step over the OLD contents: %s)" % (which, k, int((got[k] != want[k]).sum()), torch.equal(got[k], first[k]))


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("which", list(CACHES))
def test_a_table_allocated_where_a_freed_one_lay_is_not_served_its_entry(which, dtype):
    """build the cache for A, step, drop A; A2 allocated afresh (same shape and dtype: the allocator may hand out A's block); the
    next step equals a fresh engine fed A2.  Asserts the result only and prints whether the address repeated: an entry that keeps
    its table makes that impossible, one that does not depends on the allocator."""
    a, a2 = _tables(which == "pos_cache")
    A = _t(a)
    eng, fid, first, fresh = _cached_step(which, dtype, A)
    ptr = A.data_ptr()
    del A
    A2 = _t(a2)
    print("\n[table caches %s %s] the new table %s the freed one's address" % (which, dtype, "got" if A2.data_ptr() == ptr else "did not get"))
    got = _step(eng, A2, fid)
    want = _step(fresh(), A2, fid)
    torch.cuda.synchronize()
    assert not _same(first, want)
    for k in WHAT:
        assert torch.equal(got[k], want[k]), "%s: %s differs from a fresh engine's in %d elements (address repeated: %s)" % (
            which, k, int((got[k] != want[k]).sum()), A2.data_ptr() == ptr)


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_frozen_cache_and_views_of_the_table(dtype):
    """A table of 451 rows passed whole (hit), then as big[:401] - same address, fewer rows: not the whole table's entry, the pass
    recomputes and equals a fresh engine's - then as big[:] (a view of the whole, unchanged table: hit again)."""
    a, _ = _tables(False)
    big = _t(np.concatenate([a, a[1:51]], 0))
    assert big.shape[0] == 451
    eng, fid, first, fresh = _cached_step("fcache", dtype, big)
    calls = _count_embed(eng)
    part = big[:401]
    assert part.data_ptr() == big.data_ptr() and part.shape[0] < big.shape[0]
    got = _step(eng, part, fid)
    assert len(calls) == 1, "a view with fewer rows was served the whole table's frozen cache"
    assert _same(got, _step(fresh(), part, fid)) and _same(got, first)            # the same news under the same indices
    del calls[:]
    whole = big[:]
    assert whole is not big and whole.shape == big.shape
    assert _same(_step(eng, whole, fid), first) and not calls                     # a hit: no embedding launch
    assert eng.fcache[4] is big


def test_position_ids_and_views_of_the_table():
    """The same for _pos_ids, the hits asserted by identity of the returned ids: big (451 rows) caches; big[:] hits; big[:401] (more
    than 4 N_alloc rows itself) gets ids of its own shape, equal to the whole table's first rows; a per-step batch is never cached."""
    a, _ = _tables(True)
    big = _t(np.concatenate([a, a[1:51]], 0))
    eng = _engine("fp16", HR.B_SHORT, pos_pad_id=POS_PAD)
    pid = eng._pos_ids(big)
    assert eng._pos_cache is not None and eng._pos_cache[1] is pid and eng._pos_cache[2] is big
    ids = big[:, :HR.L].long()
    ne = ids != POS_PAD
    assert torch.equal(pid.long(), torch.cumsum(ne.long(), 1) * ne + POS_PAD) and pid.dtype == torch.int32      # the definition
    assert eng._pos_ids(big) is pid and eng._pos_ids(big[:]) is pid and eng._pos_ids(big.view(451, 2 * HR.L)) is pid
    part = eng._pos_ids(big[:401])
    assert part is not pid and part.shape == (401, HR.L) and torch.equal(part, pid[:401])
    assert eng._pos_cache[2].shape[0] == 401 and eng._pos_ids(big[:401]) is part                                # the one entry moved on
    small = eng._pos_ids(big[:50])
    assert small.shape == (50, HR.L) and eng._pos_ids(big[:401]) is part                                        # a batch is not cached
    big[7, 1] = POS_PAD                                                                                         # one token becomes a pad
    again = eng._pos_ids(big[:401])
    assert again is not part and int(again[7, 1]) == POS_PAD and int(part[7, 1]) != POS_PAD
