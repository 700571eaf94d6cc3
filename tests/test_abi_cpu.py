"""CPU: the C-ABI library loads and exports every symbol include/tnr_hip.h declares (no compute calls)."""
import ctypes
import os
import re

import pytest

import tnr_hip as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_symbols_are_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "tnr_hip.h")).read()
    declared = set(re.findall(r"\b(tnr_[a-z0-9_]+)\s*\(", hdr))
    assert declared, "no declarations parsed"
    lib = ctypes.CDLL(T.LIB_PATH)
    for name in sorted(declared):
        assert hasattr(lib, name), "libtnr_hip.so does not export %s" % name
    assert declared == set(T.EXPORTS), declared ^ set(T.EXPORTS)


def test_library_never_switches_or_drains_a_device():
    """include/tnr_hip.h: the library never calls hipSetDevice / hipDeviceSynchronize / hipStreamSynchronize (the caller's current
    device rules, nothing blocks the host) -- checked on the dynamic symbol table of the shipped .so; and it exports no test
    hook (those live in libtnr_testhooks.so)."""
    import subprocess
    out = subprocess.run(["nm", "-D", "--undefined-only", T.LIB_PATH], capture_output=True, text=True, check=True).stdout
    undefined = set(re.findall(r"\bU\s+(\w+)", out))
    assert "hipLaunchKernel" in undefined or any(u.startswith("hipLaunch") or u.startswith("__hipPushCallConfiguration") for u in undefined)
    for banned in ("hipSetDevice", "hipDeviceSynchronize", "hipStreamSynchronize", "hipDeviceReset", "hipMalloc", "hipFree"):
        assert banned not in undefined, "libtnr_hip.so imports %s" % banned
    exported = subprocess.run(["nm", "-D", "--defined-only", T.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "tnr_debug" not in exported
    hooks = os.path.join(os.path.dirname(T.LIB_PATH), "libtnr_testhooks.so")
    assert os.path.exists(hooks) and hasattr(ctypes.CDLL(hooks), "tnr_debug_cu_hog")


def test_build_switch_is_tested_in_common_h_only():
    """Which sources are built twice (bf16 and -DTNR_BUILD_F16) is a fact of the Makefile's TYPED / ONCE lists: no source fences
    part of itself off for one of the two builds, csrc/common.h alone maps the switch to the 16-bit type and the entry-point names."""
    import glob
    csrc = os.path.join(ROOT, "tiny-newsrec_amd", "csrc")
    files = sorted(f for ext in ("*.hip", "*.cpp", "*.h") for f in glob.glob(os.path.join(csrc, ext)))
    assert len(files) >= 10 and os.path.join(csrc, "common.h") in files
    users = [os.path.basename(f) for f in files if "TNR_BUILD_F16" in open(f).read()]
    assert users == ["common.h"], users


def test_version_without_gpu():
    assert T.query("tnr_version") == 1


def test_missing_library_fails_loudly(monkeypatch):
    """No CPU / eager fallback anywhere on the product path: without libtnr_hip.so the first engine call raises."""
    import engine as E
    import tnr_hip as T
    monkeypatch.setattr(T, "_lib", None)
    monkeypatch.setattr(T, "LIB_PATH", "/nonexistent/libtnr_hip.so")
    with pytest.raises(T.TnrError, match="not built"):
        E.Engine(E.EngineConfig(n_layers=1, trainable_layers=(0,), num_teachers=1), device="cpu", max_batch=1)


def _plan(M, N, flags=0, n_cu=256):
    mi, P, x = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    rc = T.lib().tnr_gemm_nt_plan(M, N, flags, n_cu, ctypes.cast(ctypes.byref(mi), ctypes.c_void_p),
                                  ctypes.cast(ctypes.byref(P), ctypes.c_void_p), ctypes.cast(ctypes.byref(x), ctypes.c_void_p))
    assert rc == 0
    return mi.value, P.value, x.value


def test_gemm_row_tiling_covers_every_row_exactly_once():
    """Host logic of the persistent NT kernel (csrc/gemm_plan.hip:pp_plan, csrc/gemm.hip:pp_panel): P row panels, x of them 32*mi rows and the rest
    32 rows shorter, spread evenly.  The panels must tile [0, >= M) without gaps or overlaps for every shape, and the column
    sums' partial rows are counted per 256-row panel (tnr_gemm_colsum_rows), so a COLSUM launch keeps the uniform tiling."""
    import random
    rnd = random.Random(5)
    shapes = [(52800, 768), (52800, 2304), (52800, 3072), (52800, 256), (1, 256), (129, 768), (3300, 3072)]
    shapes += [(rnd.randint(129, 120000), 256 * rnd.randint(1, 12)) for _ in range(300)]
    for M, N in shapes:
        for n_cu in (256, 304, 64):
            mi, P, x = _plan(M, N, 0, n_cu)
            assert mi in (7, 8) and 0 <= x <= P and P >= 1, (M, N, mi, P, x)
            tall, short = 32 * mi, 32 * mi - 32
            start, rows = 0, 0
            for p in range(P):
                a, b = (p * x) // P, ((p + 1) * x) // P
                assert short * p + 32 * a == start, (M, N, p)          # pp_panel's closed form == running sum
                h = tall if b > a else short
                start += h
            assert start == x * tall + (P - x) * short >= M, (M, N, mi, P, x)
            assert start - M < tall + short, (M, N, mi, P, x)           # never more than the last panels' slack
        mi, P, x = _plan(M, N, T.EPI_COLSUM)
        assert (mi, P, x) == (8, (M + 255) // 256, (M + 255) // 256)
        assert 4 * P == T.query("tnr_gemm_colsum_rows", M)
    # the headline step's shapes fill whole rounds of 256 workgroups
    assert _plan(52800, 768) == (7, 256, 114)
    assert _plan(52800, 2304)[0:2] == (8, 227)


def test_tile_queue_register_guard():
    """tools/check_pending_spill.py: the persistent GEMMs keep a queue answer in flight in a register the compiler does not know is
    pending (csrc/gemm.hip: pp_q_fetch / pp_q_wait).  The guard follows every fetch through the kernel's control-flow graph and
    fails on ANY instruction that touches the register before an executed s_waitcnt vmcnt(0): its self-test (scratch spill, AGPR
    spill, v_mov copy, v_readfirstlane, a register range, a clobber - each on a path that branches AROUND a wait) and the shipped
    objects of both builds."""
    import subprocess
    import sys
    tool = os.path.join(ROOT, "tools", "check_pending_spill.py")
    r = subprocess.run([sys.executable, tool, "--selftest"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    objs = [os.path.join(os.path.dirname(T.LIB_PATH), f) for f in ("gemm.o", "gemm_f16.o")]
    if all(os.path.exists(o) for o in objs):                      # objects are build products: present wherever build() has run
        r = subprocess.run([sys.executable, tool] + objs, capture_output=True, text=True)
        assert r.returncode == 0 and "in-flight fetches followed" in r.stdout, r.stdout + r.stderr
        assert int(re.search(r"(\d+) in-flight fetches", r.stdout).group(1)) >= 90
