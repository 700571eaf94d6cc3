"""CPU: the split dropout entry points refuse sites that cannot be the two halves of one pass pair, and split rows outside
[0, M], before anything reaches a device (argument checks only; no pointer is dereferenced)."""
import ctypes

import pytest

import tnr_hip as T

TNR_EINVAL = -1                    # include/tnr_hip.h
BUF = 1 << 20                      # a 16-byte aligned stand-in address: the calls below return before touching it


def _sites():
    return T.Dropout.site_of(0.1, 99, T.DROP_FFN_OUT, 1, 4), T.Dropout.site_of(0.1, 99, T.DROP_FFN_OUT, 1, 5)


def _gemm(name, head, tail, split, M=64):
    fn = getattr(T.lib(), name)
    return fn(BUF, 768, BUF, 768, BUF, 768, M, 768, 768, None, BUF, 768, None, 0, T.EPI_RES, None,
              ctypes.byref(head), ctypes.byref(tail) if tail is not None else None, split, None)


def _ln(name, head, tail, split, M=64):
    fn = getattr(T.lib(), name)
    return fn(BUF, BUF, BUF, BUF, BUF, None, None, None, BUF, M, 768, BUF, ctypes.byref(head),
              ctypes.byref(tail) if tail is not None else None, split, None)


@pytest.mark.parametrize("name,call", [("tnr_gemm_nt_do_split", _gemm), ("tnr_gemm_nt_do_split_f16", _gemm),
                                       ("tnr_ln_bwd_do_split", _ln), ("tnr_ln_bwd_do_split_f16", _ln)])
def test_mismatched_split_sites_return_einval(name, call):
    head, tail = _sites()
    for bad in (T.Dropout(tail.seed + 1, tail.site, tail.call, tail.p), T.Dropout(tail.seed, tail.site + 1, tail.call, tail.p),
                T.Dropout(tail.seed, tail.site, tail.call, 0.2)):
        assert call(name, head, bad, 32) == TNR_EINVAL
        assert b"share seed, site and p" in T.lib().tnr_last_error()
    for split in (-1, 65):
        assert call(name, head, tail, split) == TNR_EINVAL
        assert b"split row" in T.lib().tnr_last_error()


def test_mask_dump_split_row_checked():
    head, tail = _sites()
    L = T.lib()
    assert L.tnr_dropout_mask_split(ctypes.byref(head), ctypes.byref(tail), 11, 10, 768, BUF, None) == TNR_EINVAL
    assert b"split row" in L.tnr_last_error()
