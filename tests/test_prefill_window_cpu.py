"""CPU tests of the fp8 cache's windowed prefill call: the interface, the host refusals (every host check runs
before any HIP call, so dummy pointers reach them), the kernel instances and the contract's restatement
(tests/prefill_window_ref.py) against float64."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tests import decode_window_ref as dwr
from tests import fp8_ref
from tests import prefill_window_ref as ref
from tests import rect_ref as rr
from tests.test_fp8_cpu import CAUSAL, DUMMY, FP8, V1A, lib, make  # noqa: F401

CALL, PAGED = "qmha_attend_cached_prefill_window", "qmha_attend_cached_paged_prefill_window"


def test_interface(lib):
    from quantizedmha_amd import _lib, torch_ext
    i, vp = ctypes.c_int, ctypes.c_void_p
    assert _lib.SIGNATURES[CALL] == (i, [vp, vp, vp, i, vp, i, vp, ctypes.c_uint, vp])
    assert _lib.SIGNATURES[PAGED] == (i, [vp, vp, vp, i, vp, vp, i, vp, ctypes.c_uint, vp])
    header = open(_lib.HERE + "/../include/launchers.h").read()
    assert all(f" {name}(" in header and hasattr(lib, name) for name in (CALL, PAGED))
    assert hasattr(torch_ext.KVCache, "attend_prefill_window") and hasattr(torch_ext.GroupedKVCache, "attend_prefill_window")
    assert hasattr(torch_ext.PagedKVCache, "attend_paged_prefill_window")


def test_host_refusals(lib):
    def refused(st, status, *words):
        msg = lib.qmha_last_error().decode()
        assert st == status and all(w in msg for w in words), (st, msg)

    c, p, f16 = make(lib), make(lib, paged=True), make(lib, V1A)
    a, call, paged = (DUMMY, DUMMY, 1, DUMMY), getattr(lib, CALL), getattr(lib, PAGED)
    for window in (0, -32):
        refused(call(c, *a, window, None, CAUSAL, None), 1, "attend_prefill_window", f"window = {window}", "window >= 1")
    refused(paged(p, *a, DUMMY, 0, None, CAUSAL, None), 1, "attend_paged_prefill_window", "window = 0")
    refused(call(f16, *a, 64, None, CAUSAL, None), 4, "attend_prefill_window", "fa_tc_v1a", "attend_tokens_window")
    refused(call(c, *a, 64, None, 0, None), 1, "QMHA_FLAG_CAUSAL")
    for nq in (0, -1, 257):
        refused(call(c, DUMMY, DUMMY, nq, DUMMY, 64, None, CAUSAL, None), 1, f"Nq = {nq} rows", "1 <= Nq <= cap = 256")
    refused(call(c, DUMMY, DUMMY, 1, None, 64, None, CAUSAL, None), 1, "null lens")
    refused(call(c, None, DUMMY, 1, DUMMY, 64, None, CAUSAL, None), 1, "null tensor pointer")
    refused(paged(p, *a, None, 64, None, CAUSAL, None), 1, "null table")
    refused(call(p, *a, 64, None, CAUSAL, None), 1, "attend_prefill_window", "the cache is paged")
    refused(paged(c, *a, DUMMY, 64, None, CAUSAL, None), 1, "attend_paged_prefill_window", "the cache is contiguous")
    for x in (c, p, f16):
        lib.qmha_kv_cache_destroy(x)


def test_four_instances(lib):
    path = os.path.join(os.path.dirname(fp8_ref.__file__), "..", "quantizedmha_amd", "lib", "libqmha.so")
    syms = subprocess.run(["nm", "-C", path], capture_output=True, text=True, check=True).stdout
    got = sorted(set(re.findall(r"__device_stub__(qmha_fp8_band_kernel<.*?>)\(", syms)))
    assert got == sorted(f"qmha_fp8_band_kernel<qmha::{g}, {d}>" for g in ("Ragged", "Paged") for d in (64, 128)), got


@pytest.mark.parametrize("nq,L,window", [(1, 100, 33), (33, 65, 1), (70, 193, 100), (100, 193, 31), (100, 224, 64), (70, 224, 1000)])
def test_restatement_against_float64(nq, L, window):
    """fp8_ref's bound: each p within 2^-4 of its value or lost below 2^-10 of its base 2^8 -- the sink only scales those terms
    down --, so O is within (2^-4 + L 2^-18) max|v| of float64 band-plus-sink attention on the same e4m3 operands."""
    D, scales, sinks = 64, (0.3, 0.7, 1.9), np.array([1.5])
    Q, K, V = rr.inputs(nq, 224, D, 1, "normal", 5)
    O, Ltot, vmax = ref.prefill_window(Q, K, V, [L], 1, 1, scales, 224, window, sinks)
    k8, _, v8 = fp8_ref.cache_arrays(K[0], V[0], L, scales[1], scales[2])
    q, k, v = (fp8_ref.decode(x).astype(np.float64)[None] * s for x, s in zip((fp8_ref.encode(Q[0], scales[0]), k8, v8), scales))
    want = dwr.exact(q, k, v, [L], 1, 1, window, sinks)
    assert np.isfinite(O).all() and (Ltot > 0).all()
    assert np.abs(O - want).max() <= (2.0 ** -4 + L * 2.0 ** -18) * vmax[0, 0]
