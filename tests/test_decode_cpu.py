"""CPU tests of the fp8 cache's decode call: the interface, the scratch size, the host refusals (every host
check runs before any HIP call, so dummy pointers reach them), the kernel instances and the contract's restatement
(tests/decode_ref.py) against float64."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tests import decode_ref, fp8_ref
from tests import rect_ref as rr
from tests.test_fp8_cpu import CAUSAL, DUMMY, FP8, MEM, V1A, lib, make  # noqa: F401


def test_interface_and_scratch_bytes(lib):
    from quantizedmha_amd import _lib
    i, vp, sz = ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t
    assert _lib.SIGNATURES["qmha_attend_decode_bytes"] == (sz, [vp, i, i])
    assert _lib.SIGNATURES["qmha_attend_cached_decode"] == (i, [vp, vp, vp, i, vp, i, vp, sz, ctypes.c_uint, vp])
    assert _lib.SIGNATURES["qmha_attend_cached_paged_decode"] == (i, [vp, vp, vp, i, vp, vp, i, vp, sz, ctypes.c_uint, vp])
    c, f16 = make(lib), make(lib, V1A)  # B 2, cap 256, h 2, d 64
    for nq, chunk in ((1, 64), (5, 128), (32, 256)):
        assert lib.qmha_attend_decode_bytes(c, nq, chunk) == decode_ref.layout(2, 256 // chunk, nq, 2, 64)[1]
        assert lib.qmha_attend_decode_bytes(c, nq, chunk) == lib.qmha_attend_split_bytes(f16, nq, chunk)
    assert [lib.qmha_attend_decode_bytes(c, *a) for a in ((0, 64), (33, 64), (1, 32), (1, 96), (1, 320))] == [0] * 5
    assert lib.qmha_attend_decode_bytes(f16, 1, 64) == 0 and lib.qmha_attend_decode_bytes(None, 1, 64) == 0
    lib.qmha_kv_cache_destroy(c), lib.qmha_kv_cache_destroy(f16)


def test_host_refusals(lib):
    def refused(st, status, *words):
        msg = lib.qmha_last_error().decode()
        assert st == status and all(w in msg for w in words), (st, msg)

    c, p, f16 = make(lib), make(lib, paged=True), make(lib, V1A)
    h4 = ctypes.c_void_p()
    assert lib.qmha_kv_cache_create_gqa(ctypes.byref(h4), MEM, 1 << 30, 2, 256, 256, 4, 1, FP8) == 0
    big, a = 1 << 30, (DUMMY, DUMMY, 1, DUMMY)  # Q, O, Nq, lens
    refused(lib.qmha_attend_cached_decode(c, DUMMY, DUMMY, 33, DUMMY, 64, MEM, big, CAUSAL, None), 1, "Nq * (h / h_kv) = 33 * 1 = 33", "limit is 32",
            "attend_tokens")
    refused(lib.qmha_attend_cached_decode(h4, DUMMY, DUMMY, 9, DUMMY, 64, MEM, big, CAUSAL, None), 1, "9 * 4 = 36", "limit is 32", "attend_tokens")
    for chunk in (32, 96, 320):
        refused(lib.qmha_attend_cached_decode(c, *a, chunk, MEM, big, CAUSAL, None), 1, f"chunk_rows = {chunk}", "multiple of 64", "cap = 256")
    refused(lib.qmha_attend_cached_decode(c, *a, 64, None, big, CAUSAL, None), 1, "null scratch", "qmha_attend_decode_bytes")
    refused(lib.qmha_attend_cached_decode(c, *a, 64, ctypes.c_void_p(0x10010), big, CAUSAL, None), 1, "256-byte aligned")
    need = lib.qmha_attend_decode_bytes(c, 1, 64)
    refused(lib.qmha_attend_cached_decode(c, *a, 64, MEM, need - 1, CAUSAL, None), 1, "scratch too small", str(need))
    refused(lib.qmha_attend_cached_decode(c, *a, 64, MEM, big, 0, None), 1, "QMHA_FLAG_CAUSAL")
    refused(lib.qmha_attend_cached_decode(c, DUMMY, DUMMY, 1, None, 64, MEM, big, CAUSAL, None), 1, "null lens")
    refused(lib.qmha_attend_cached_paged_decode(p, *a, None, 64, MEM, big, CAUSAL, None), 1, "null table")
    refused(lib.qmha_attend_cached_decode(p, *a, 64, MEM, big, CAUSAL, None), 1, "attend_decode", "the cache is paged")
    refused(lib.qmha_attend_cached_paged_decode(c, *a, DUMMY, 64, MEM, big, CAUSAL, None), 1, "attend_paged_decode", "the cache is contiguous")
    refused(lib.qmha_attend_cached_decode(f16, *a, 64, MEM, big, CAUSAL, None), 4, "attend_decode", "fa_tc_v1a", "attend_tokens_split")
    for x in (c, p, f16, h4):
        lib.qmha_kv_cache_destroy(x)


def test_eight_instances(lib):
    syms = subprocess.run(["nm", "-C", os.path.join(os.path.dirname(fp8_ref.__file__), "..", "quantizedmha_amd", "lib", "libqmha.so")], capture_output=True, text=True, check=True).stdout
    got = sorted(set(re.findall(r"__device_stub__(qmha_fp8_decode_kernel<.*?>)\(", syms)))
    assert got == sorted(f"qmha_fp8_decode_kernel<qmha::{g}, {d}, {qb}>" for g in ("Ragged", "Paged") for d in (64, 128) for qb in (1, 2)), got


@pytest.mark.parametrize("nq,L,chunk", [(1, 100, 64), (5, 65, 64), (8, 193, 128)])
def test_restatement_against_float64(nq, L, chunk):
    """fp8_ref's bound: each p within 2^-4 of its value or lost below 2^-10 of its stream's base 2^8 -- the merge and the combine
    only scale those terms down --, so O is within (2^-4 + L 2^-18) max|v| of float64 attention on the same e4m3 operands."""
    D, scales = 64, (0.3, 0.7, 1.9)
    Q, K, V = rr.inputs(nq, 224, D, 1, "normal", 5)
    O, (Oc, m, l), Ltot, vmax = decode_ref.decode(Q, K, V, [L], 1, 1, scales, chunk, 224)
    k8, _, v8 = fp8_ref.cache_arrays(K[0], V[0], L, scales[1], scales[2])
    q, k, v = (fp8_ref.decode(x).astype(np.float64) for x in (fp8_ref.encode(Q[0], scales[0]), k8, v8))
    s = (q @ k[:L].T) * scales[0] * scales[1] / np.sqrt(D)
    s[np.arange(L)[None, :] > (np.arange(nq) + L - nq)[:, None]] = -np.inf
    p = np.exp(s - s.max(axis=1, keepdims=True))
    want = scales[2] * (p @ v[:L]) / p.sum(axis=1, keepdims=True)
    assert np.abs(O[0] - want).max() <= (2.0 ** -4 + L * 2.0 ** -18) * vmax[0, 0]
    written = ~np.isnan(l[0, :, :, 0])  # row r has chunk c iff c <= ((L - nq + r) / 32) / C
    assert np.array_equal(written, np.arange(l.shape[1])[:, None] <= ((L - nq + np.arange(nq)) // 32 // (chunk // 32))[None, :])
