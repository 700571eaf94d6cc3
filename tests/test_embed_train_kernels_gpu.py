"""GPU: the two kernels behind --train_embeddings through the C ABI, both 16-bit builds, against float64 references computed here.

tnr_embed_ln_bwd / tnr_embed_ln_bwd_indexed: float64 autograd of LayerNorm(word[id] + pos[pi] + type0) * mask (the forward of
tests/dropout_ref.embed_ln); the mask is oracle/dropout_oracle.py's, as in tests/test_dropout_kernels_gpu.py.
tnr_scatter_sum_rows: float64 index_add, to the recursive-summation bound count * 2^-23 * sum |terms|, and bit-identical twice."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import tnr_hip as T                              # noqa: E402
from oracle import dropout_oracle as DO          # noqa: E402
from dropout_ref import roberta_pos_ids          # noqa: E402

DEV = "cuda:0"
VOCAB, EPS, SEED, CALL = 64, 1e-12, 1234, 7
TDT = {"bf16": torch.bfloat16, "fp16": torch.float16}


def _name(n, dtype):
    return n + ("_f16" if dtype == "fp16" else "")


def _tokens(n_seq, L, indexed):
    """-> (token table rows [ids | mask] (rows, 2L), nidx or None, ids of the encoded sequences (n_seq, L))."""
    rng = np.random.RandomState(100 * n_seq + L)
    rows = n_seq + 3 if indexed else n_seq
    ids = rng.randint(1, VOCAB, size=(rows, L))
    lens = rng.randint(2, L + 1, size=rows)
    for r in range(rows):
        ids[r, lens[r]:] = 0                     # pad id 0 present
    ids[0, 0] = 0
    ids[-1, 1] = VOCAB - 1                       # the table's last row
    tok = np.concatenate([ids, (ids != 0).astype(ids.dtype)], 1)
    if not indexed:
        return tok, None, ids
    nidx = rng.randint(0, rows, size=n_seq)
    nidx[0], nidx[-1] = rows - 1, rows - 1       # a repeated news row
    if n_seq > 2:
        nidx[1] = 0
    return tok, nidx.astype(np.int32), ids[nidx]


def _reference(ids, pi, word, pos, type0, gamma, dy, mask):
    """float64 autograd -> (dx (n_tok, H), dgamma, dbeta) of sum(dy * LN(word[id] + pos[pi] + type0) * mask)."""
    f = lambda a: torch.from_numpy(np.asarray(a, np.float64))
    x = (f(word)[torch.from_numpy(ids).long()] + f(pos)[torch.from_numpy(pi).long()] + f(type0)).reshape(-1, word.shape[1])
    x.requires_grad_(True)
    g, b = f(gamma).requires_grad_(True), torch.zeros(word.shape[1], dtype=torch.float64, requires_grad=True)
    y = torch.nn.functional.layer_norm(x, (word.shape[1],), g, b, EPS)
    if mask is not None:
        y = y * f(mask)
    (y * f(dy)).sum().backward()
    return x.grad.numpy(), g.grad.numpy(), b.grad.numpy()


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("indexed", [False, True], ids=["rows", "indexed"])
@pytest.mark.parametrize("H", [256, 768])
@pytest.mark.parametrize("shape", [(5, 30), (3, 33), (2, 512)], ids=lambda s: "%dx%d" % s)
def test_embed_ln_bwd_matches_float64_autograd(shape, H, indexed, dtype):
    """(5, 30): 150 tokens, not a multiple of the 4 tokens a block takes per turn nor of its 16; (3, 33): a padded mask row;
    (2, 512): the long form.  Each with pos_ids NULL / given, p = 0.1 / 0 and inv_scale 1 / 2^-10."""
    n_seq, L = shape
    n_tok = n_seq * L
    rng = np.random.RandomState(H + n_tok)
    tok, nidx, ids = _tokens(n_seq, L, indexed)
    word = rng.randn(VOCAB, H).astype(np.float32)
    pos = rng.randn(L + 2, H).astype(np.float32)
    type0 = rng.randn(H).astype(np.float32)
    gamma = (1.0 + 0.3 * rng.randn(H)).astype(np.float32)
    dy16 = torch.from_numpy(rng.randn(n_tok, H).astype(np.float32)).to(TDT[dtype])
    dy = dy16.float().numpy()                    # the values the kernel reads
    dev = lambda a, dt=None: torch.from_numpy(np.ascontiguousarray(a)).to(DEV) if dt is None else \
        torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dt)
    tok_d = dev(tok, torch.int32 if indexed else torch.int64)
    nidx_d = dev(nidx) if indexed else None
    pid_tab = roberta_pos_ids(tok[:, :L], 1).astype(np.int32)          # laid out like the token table
    wd, pd, td, gd, dyd = dev(word), dev(pos), dev(type0), dev(gamma), dy16.to(DEV)
    nblk = T.query("tnr_embed_ln_bwd_blocks", n_tok)
    assert T.query("tnr_embed_ln_bwd_part_elems", n_tok, H) >= nblk * 2 * H

    def run(pid, site, inv_scale):
        dx = torch.full((n_tok, H), float("nan"), device=DEV)
        part = torch.full((nblk, 2 * H), float("nan"), device=DEV)
        gb = torch.zeros(2 * H, device=DEV)
        tail = (dyd, wd, pd, td, gd, EPS, inv_scale, dx, part, site, pid)
        if indexed:
            T.call(_name("tnr_embed_ln_bwd_indexed", dtype), tok_d, nidx_d, n_seq, L, H, *tail)
        else:
            T.call(_name("tnr_embed_ln_bwd", dtype), tok_d, n_seq, L, H, *tail)
        T.call("tnr_reduce_rows", part, nblk, 2 * H, 2 * H, gb, 0)
        torch.cuda.synchronize()
        return dx.cpu().numpy(), gb.cpu().numpy()

    for with_pid in (False, True):
        pid_d = dev(pid_tab) if with_pid else None
        pi = (pid_tab[nidx] if indexed else pid_tab) if with_pid else np.arange(L)[None, :].repeat(n_seq, 0)
        base = None
        for p in (0.0, 0.1):
            mask = DO.rows_mask(p, SEED, T.DROP_EMB, CALL, n_tok, H) if p > 0 else None
            site = T.Dropout(SEED, T.DROP_EMB, CALL, p)
            dx_ref, dg_ref, db_ref = _reference(ids, pi, word, pos, type0, gamma, dy, mask)
            dx, gb = run(pid_d, site, 1.0)
            err = np.abs(dx - dx_ref).max() / np.abs(dx_ref).max()
            print("\n[%s H=%d %dx%d %s pos_ids=%d p=%.1f] dx max|err| / max|ref| %.2e ; dgamma %.2e dbeta %.2e (abs)" %
                  (dtype, H, n_seq, L, "indexed" if indexed else "rows", with_pid, p, err,
                   np.abs(gb[:H] - dg_ref).max(), np.abs(gb[H:] - db_ref).max()))
            np.testing.assert_allclose(dx, dx_ref, rtol=1e-4, atol=1e-4 * np.abs(dx_ref).max())
            np.testing.assert_allclose(gb[:H], dg_ref, rtol=1e-3, atol=1e-3)
            np.testing.assert_allclose(gb[H:], db_ref, rtol=1e-3, atol=1e-3)
            if p == 0.0:
                dx0, gb0 = run(pid_d, None, 1.0)                       # a site with p = 0 is no site: the same bits
                assert np.array_equal(dx, dx0) and np.array_equal(gb, gb0)
                base = dx
            # the loss scale leaves exactly: a power of two on dx, nothing on the partials (their reduction carries it)
            dxs, gbs = run(pid_d, site, 2.0 ** -10)
            assert np.array_equal(dxs, dx * np.float32(2.0 ** -10)) and np.array_equal(gbs, gb)
        assert base is not None


def _scatter_case(D, rng):
    """700 keys with runs of length 1, 3, 5, 70 and 300, the skip key as the longest run (310) and keys outside the table."""
    rows = 40
    runs = [(3, 300), (17, 70), (5, 5), (9, 3), (11, 1), (39, 1), (0, 1), (21, 4), (22, 2), (8, 310), (rows + 5, 1), (-1, 2)]
    keys = np.concatenate([np.full(c, k) for k, c in runs]).astype(np.int32)
    assert keys.size == 700
    keys = keys[rng.permutation(keys.size)]
    src = rng.randn(keys.size, D).astype(np.float32)
    return rows, 8, keys, src


@pytest.mark.parametrize("D", [256, 768])
def test_scatter_sum_rows_against_float64_index_add(D):
    rng = np.random.RandomState(D)
    rows, skip, keys, src = _scatter_case(D, rng)
    kd = torch.from_numpy(keys).to(DEV)
    ks, order = torch.sort(kd, stable=True)
    order = order.to(torch.int32)
    sd = torch.from_numpy(src).to(DEV)
    ok = (keys != skip) & (keys >= 0) & (keys < rows)
    want = np.zeros((rows, D), np.float64)
    bound = np.zeros((rows, D), np.float64)
    np.add.at(want, keys[ok], src[ok].astype(np.float64))
    np.add.at(bound, keys[ok], np.abs(src[ok]).astype(np.float64))
    count = np.bincount(keys[ok], minlength=rows).astype(np.float64)[:, None]
    named = count[:, 0] > 0
    assert {1, 3, 5, 70, 300} <= set(count[:, 0].astype(int)) and not named[skip]
    SENT = np.float32(-7.25)
    outs = []
    for acc in (0, 1, 1, 0):
        table = torch.full((rows + 1, D), float(SENT), device=DEV)               # one guard row behind the table
        T.call("tnr_scatter_sum_rows", sd, keys.size, D, ks, order, skip, table, rows, acc)
        torch.cuda.synchronize()
        got = table.cpu().numpy()
        assert (got[rows] == SENT).all() and (got[:rows][~named] == SENT).all()   # rows no key names, the skip row, the guard
        w = want + (float(SENT) if acc else 0.0)
        b = (count + acc) * 2.0 ** -23 * (bound + (abs(float(SENT)) if acc else 0.0))
        err = np.abs(got[:rows].astype(np.float64) - w)
        print("\n[scatter D=%d accumulate=%d] worst err / bound %.3f" % (D, acc, (err[named] / b[named]).max()))
        assert (err[named] <= b[named]).all()
        outs.append(got)
    assert np.array_equal(outs[1], outs[2]) and np.array_equal(outs[0], outs[3])   # two calls give equal bits
