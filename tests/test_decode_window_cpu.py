"""CPU tests of the fp8 cache's windowed decode call: the interface, the scratch size and the chunk count NCw
against every valid length, the host refusals (every host check runs before any HIP call, so dummy pointers reach them) and
the contract's restatement (tests/decode_window_ref.py) against float64."""
import ctypes

import numpy as np
import pytest

from tests import decode_window_ref as ref
from tests import fp8_ref
from tests import rect_ref as rr
from tests.test_fp8_cpu import CAUSAL, DUMMY, FP8, MEM, V1A, lib, make  # noqa: F401

WINDOWS = (1, 31, 32, 33, 64, 100, 224, 1000)
BYTES, CALL, PAGED = "qmha_attend_decode_window_bytes", "qmha_attend_cached_decode_window", "qmha_attend_cached_paged_decode_window"


def test_interface(lib):
    from quantizedmha_amd import _lib
    i, vp, sz = ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t
    assert _lib.SIGNATURES[BYTES] == (sz, [vp, i, i, i])
    assert _lib.SIGNATURES[CALL] == (i, [vp, vp, vp, i, vp, i, vp, i, vp, sz, ctypes.c_uint, vp])
    assert _lib.SIGNATURES[PAGED] == (i, [vp, vp, vp, i, vp, vp, i, vp, i, vp, sz, ctypes.c_uint, vp])
    header = open(_lib.HERE + "/../include/launchers.h").read()
    assert all(f" {name}(" in header and hasattr(lib, name) for name in (BYTES, CALL, PAGED))
    c, f16 = make(lib), make(lib, V1A)  # B 2, cap 256, h 2, d 64
    assert [lib.qmha_attend_decode_window_bytes(c, *a) for a in ((0, 64, 64), (33, 64, 64), (1, 0, 64), (1, -5, 64), (1, 64, 32), (1, 64, 320))] == [0] * 6
    assert lib.qmha_attend_decode_window_bytes(f16, 1, 64, 64) == 0 and lib.qmha_attend_decode_window_bytes(None, 1, 64, 64) == 0
    assert lib.qmha_attend_decode_window_bytes(c, 5, 2 ** 31 - 1, 64) == lib.qmha_attend_decode_bytes(c, 5, 64)  # never above the full sweep's
    lib.qmha_kv_cache_destroy(c), lib.qmha_kv_cache_destroy(f16)


@pytest.mark.parametrize("chunk", [64, 128])
@pytest.mark.parametrize("nq", [1, 5, 8])
def test_chunk_count_covers_every_length_and_no_smaller_one_does(lib, nq, chunk):
    cap, C, h = 224, chunk // 32, ctypes.c_void_p()
    assert lib.qmha_kv_cache_create(ctypes.byref(h), MEM, 1 << 30, 2, cap, 128, 2, FP8) == 0
    for window in WINDOWS:
        need = max(-(-((L - 1) // 32 - ref.first_tile(L, nq, window) + 1) // C) for L in range(nq, cap + 1))
        assert ref.chunks(cap, nq, window, chunk) == need <= -(-cap // chunk), (window, need)
        assert lib.qmha_attend_decode_window_bytes(h, nq, window, chunk) == ref.layout(2, need, nq, 2, 64)[1], window
    lib.qmha_kv_cache_destroy(h)


def test_host_refusals(lib):
    def refused(st, status, *words):
        msg = lib.qmha_last_error().decode()
        assert st == status and all(w in msg for w in words), (st, msg)

    c, p, f16 = make(lib), make(lib, paged=True), make(lib, V1A)
    h4 = ctypes.c_void_p()
    assert lib.qmha_kv_cache_create_gqa(ctypes.byref(h4), MEM, 1 << 30, 2, 256, 256, 4, 1, FP8) == 0
    big, a, call, paged = 1 << 30, (DUMMY, DUMMY, 1, DUMMY), lib.qmha_attend_cached_decode_window, lib.qmha_attend_cached_paged_decode_window
    refused(call(c, DUMMY, DUMMY, 33, DUMMY, 64, None, 64, MEM, big, CAUSAL, None), 1, "Nq * (h / h_kv) = 33 * 1 = 33", "limit is 32")
    refused(call(h4, DUMMY, DUMMY, 9, DUMMY, 64, None, 64, MEM, big, CAUSAL, None), 1, "9 * 4 = 36", "limit is 32")
    for window in (0, -32):
        refused(call(c, *a, window, None, 64, MEM, big, CAUSAL, None), 1, f"window = {window}", "window >= 1")
    for chunk in (32, 96, 320):
        refused(call(c, *a, 64, None, chunk, MEM, big, CAUSAL, None), 1, f"chunk_rows = {chunk}", "multiple of 64", "cap = 256")
    refused(call(c, *a, 64, None, 64, None, big, CAUSAL, None), 1, "null scratch", BYTES)
    refused(call(c, *a, 64, None, 64, ctypes.c_void_p(0x10010), big, CAUSAL, None), 1, "256-byte aligned")
    need = lib.qmha_attend_decode_window_bytes(c, 1, 64, 64)
    refused(call(c, *a, 64, None, 64, MEM, need - 1, CAUSAL, None), 1, "scratch too small", str(need))
    refused(call(c, *a, 64, None, 64, MEM, big, 0, None), 1, "QMHA_FLAG_CAUSAL")
    refused(call(c, DUMMY, DUMMY, 1, None, 64, None, 64, MEM, big, CAUSAL, None), 1, "null lens")
    refused(call(c, None, DUMMY, 1, DUMMY, 64, None, 64, MEM, big, CAUSAL, None), 1, "null tensor pointer")
    refused(paged(p, *a, None, 64, None, 64, MEM, big, CAUSAL, None), 1, "null table")
    refused(call(p, *a, 64, None, 64, MEM, big, CAUSAL, None), 1, "attend_decode_window", "the cache is paged")
    refused(paged(c, *a, DUMMY, 64, None, 64, MEM, big, CAUSAL, None), 1, "attend_paged_decode_window", "the cache is contiguous")
    refused(call(f16, *a, 64, None, 64, MEM, big, CAUSAL, None), 4, "attend_decode_window", "fa_tc_v1a", "attend_tokens_window")
    for x in (c, p, f16, h4):
        lib.qmha_kv_cache_destroy(x)


@pytest.mark.parametrize("nq,L,chunk,window", [(1, 100, 64, 33), (5, 65, 64, 1), (8, 193, 64, 100), (8, 193, 64, 1), (8, 193, 128, 31), (5, 224, 128, 1000)])
def test_restatement_against_float64(nq, L, chunk, window):
    """fp8_ref's bound: each p within 2^-4 of its value or lost below 2^-10 of its stream's base 2^8 -- the merge, the combine
    and the sink only scale those terms down --, so O is within (2^-4 + L 2^-18) max|v| of float64 band-plus-sink attention on
    the same e4m3 operands."""
    D, scales, sinks = 64, (0.3, 0.7, 1.9), np.array([1.5])
    Q, K, V = rr.inputs(nq, 224, D, 1, "normal", 5)
    O, (Oc, m, l), Ltot, vmax = ref.decode_window(Q, K, V, [L], 1, 1, scales, chunk, 224, window, sinks)
    k8, _, v8 = fp8_ref.cache_arrays(K[0], V[0], L, scales[1], scales[2])
    q, k, v = (fp8_ref.decode(x).astype(np.float64) for x in (fp8_ref.encode(Q[0], scales[0]), k8, v8))
    e, j = (np.arange(nq) + L - nq)[:, None], np.arange(L)[None, :]
    s = (q @ k[:L].T) * scales[0] * scales[1] / np.sqrt(D)
    s[(j > e) | (j <= e - window)] = -np.inf
    p = np.exp(s - s.max(axis=1, keepdims=True))
    want = scales[2] * (p @ v[:L]) / (p.sum(axis=1, keepdims=True) + np.exp(sinks[0] - s.max(axis=1, keepdims=True)))
    assert np.abs(O[0] - want).max() <= (2.0 ** -4 + L * 2.0 ** -18) * vmax[0, 0]
    NC, t0 = ref.chunks(224, nq, window, chunk), ref.first_tile(L, nq, window)
    assert l.shape[1] == NC and np.isfinite(O).all()
    if NC == 1:
        assert np.isnan(l).all() and np.isnan(Oc).all()  # the one-launch form leaves the scratch alone
    else:  # row r has chunk c iff c <= (((L - nq + r) / 32) - t0) / C; what exists is finite, an empty partial is l = 0
        assert np.array_equal(~np.isnan(l[0, :, :, 0]), np.arange(NC)[:, None] <= (((L - nq + np.arange(nq)) // 32 - t0) // (chunk // 32))[None, :])
        w = ~np.isnan(l)
        assert (l[w] == 0).any() == (window == 1)  # L = 193: chunk 0 is rows 128 .. 191, row 7's key 192; L = 65: rows 0 .. 63, row 4's 64
        assert np.isfinite(m[w]).all() and np.isfinite(Oc[np.repeat(w, D, axis=-1)]).all() and ((l[w] > 0) | (m[w] == ref.EMPTY_M)).all()
