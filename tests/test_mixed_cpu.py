"""CPU tests of the fp8 cache's mixed-step calls: the interface, the scratch size against the layout, the host
refusals (every host check runs before any HIP call, so dummy pointers reach them), the packed names' standing refusal of an
fp8 cache, and the two grid bounds against the true item counts."""
import ctypes

import pytest

from tests import decode_window_ref as dwr
from tests.test_fp8_cpu import CAUSAL, DUMMY, FP8, MEM, V1A, lib, make  # noqa: F401

NAMES = ("qmha_attend_mixed_bytes", "qmha_kv_cache_append_mixed", "qmha_kv_cache_append_paged_mixed", "qmha_attend_cached_mixed",
         "qmha_attend_cached_paged_mixed")


def test_interface_and_scratch_size(lib):
    from quantizedmha_amd import _lib
    i, vp, sz, u = ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint
    assert [_lib.SIGNATURES[n] for n in NAMES] == [(sz, [vp, i, i]), (i, [vp, vp, vp, i, vp, vp, vp]), (i, [vp, vp, vp, i, vp, vp, vp, vp]),
                                                   (i, [vp, vp, vp, i, vp, vp, i, vp, i, vp, sz, u, vp]),
                                                   (i, [vp, vp, vp, i, vp, vp, vp, i, vp, i, vp, sz, u, vp])]
    header = open(_lib.HERE + "/../include/launchers.h").read()
    assert all(f" {name}(" in header and hasattr(lib, name) for name in NAMES)
    c, f16, h4 = make(lib), make(lib, V1A), ctypes.c_void_p()  # B 2, cap 256, h 2, d 64
    assert lib.qmha_kv_cache_create_gqa(ctypes.byref(h4), MEM, 1 << 30, 2, 256, 256, 4, 1, FP8) == 0
    assert [lib.qmha_attend_mixed_bytes(c, *a) for a in ((0, 64), (-5, 64), (64, 32), (64, 96), (64, 320))] == [0] * 5
    assert lib.qmha_attend_mixed_bytes(f16, 64, 64) == 0 and lib.qmha_attend_mixed_bytes(None, 64, 64) == 0
    for window, chunk in ((1, 64), (33, 128), (100, 64), (2 ** 31 - 1, 64)):  # a slice of 32 / G rows, the widest decode kind's chunks
        for cache, h, G in ((c, 2, 1), (h4, 4, 4)):
            want = dwr.layout(2, dwr.chunks(256, 32 // G, window, chunk), 32 // G, h, 64)[1]
            assert lib.qmha_attend_mixed_bytes(cache, window, chunk) == want, (window, chunk, G)
    for x in (c, f16, h4):
        lib.qmha_kv_cache_destroy(x)


def test_host_refusals(lib):
    def refused(st, status, *words):
        msg = lib.qmha_last_error().decode()
        assert st == status and all(w in msg for w in words), (st, msg)

    c, p, f16 = make(lib), make(lib, paged=True), make(lib, V1A)
    big, attend, paged, append, ppaged = 1 << 30, lib.qmha_attend_cached_mixed, lib.qmha_attend_cached_paged_mixed, lib.qmha_kv_cache_append_mixed, \
        lib.qmha_kv_cache_append_paged_mixed
    a, t = (DUMMY, DUMMY, 4, DUMMY, DUMMY), (64, None, 64, MEM, big, CAUSAL, None)
    refused(attend(c, None, DUMMY, 4, DUMMY, DUMMY, *t), 1, "null tensor pointer")
    refused(attend(c, DUMMY, DUMMY, 4, None, DUMMY, *t), 1, "attend_mixed", "null cu")
    refused(attend(c, DUMMY, DUMMY, 4, DUMMY, None, *t), 1, "null lens")
    refused(paged(p, *a, None, *t), 1, "attend_paged_mixed", "null table")
    refused(attend(c, DUMMY, DUMMY, 0, DUMMY, DUMMY, *t), 1, "total = 0", "total >= 1")
    for window in (0, -32):
        refused(attend(c, *a, window, None, 64, MEM, big, CAUSAL, None), 1, f"window = {window}", "window >= 1")
    for chunk in (32, 96, 320):
        refused(attend(c, *a, 64, None, chunk, MEM, big, CAUSAL, None), 1, f"chunk_rows = {chunk}", "multiple of 64", "cap = 256")
    refused(attend(c, *a, 64, None, 64, None, big, CAUSAL, None), 1, "null scratch", NAMES[0])
    refused(attend(c, *a, 64, None, 64, ctypes.c_void_p(0x10010), big, CAUSAL, None), 1, "256-byte aligned")
    need = lib.qmha_attend_mixed_bytes(c, 64, 64)
    refused(attend(c, *a, 64, None, 64, MEM, need - 1, CAUSAL, None), 1, "scratch too small", str(need))
    refused(attend(c, *a, 64, None, 64, MEM, big, 0, None), 1, "QMHA_FLAG_CAUSAL")
    refused(attend(p, *a, *t), 1, "attend_mixed", "the cache is paged")
    refused(paged(c, *a, DUMMY, *t), 1, "attend_paged_mixed", "the cache is contiguous")
    refused(attend(f16, *a, *t), 4, "attend_mixed", "fa_tc_v1a", "attend_packed")
    refused(append(c, None, DUMMY, 4, DUMMY, DUMMY, None), 1, "null tensor pointer")
    refused(append(c, DUMMY, DUMMY, 4, None, DUMMY, None), 1, "append_mixed", "null cu")
    refused(append(c, DUMMY, DUMMY, 4, DUMMY, None, None), 1, "null pos")
    refused(append(c, DUMMY, DUMMY, -1, DUMMY, DUMMY, None), 1, "total = -1")
    refused(ppaged(p, DUMMY, DUMMY, 4, DUMMY, DUMMY, None, None), 1, "append_paged_mixed", "null table")
    refused(append(p, DUMMY, DUMMY, 4, DUMMY, DUMMY, None), 1, "the cache is paged")
    refused(ppaged(c, DUMMY, DUMMY, 4, DUMMY, DUMMY, DUMMY, None), 1, "the cache is contiguous")
    refused(append(f16, DUMMY, DUMMY, 4, DUMMY, DUMMY, None), 4, "append_mixed", "fa_tc_v1a", "append_packed")
    # the packed names keep refusing an fp8 cache
    refused(lib.qmha_kv_cache_append_packed(c, DUMMY, DUMMY, 4, 2, DUMMY, DUMMY, None), 4, "append_packed", "packed batch")
    refused(lib.qmha_attend_cached_packed(c, DUMMY, DUMMY, 4, 2, DUMMY, DUMMY, CAUSAL, None), 4, "attend_packed", "packed batch")
    refused(lib.qmha_kv_cache_append_paged_packed(p, DUMMY, DUMMY, 4, 2, DUMMY, DUMMY, DUMMY, None), 4, "packed batch")
    refused(lib.qmha_attend_cached_paged_packed(p, DUMMY, DUMMY, 4, 2, DUMMY, DUMMY, DUMMY, CAUSAL, None), 4, "packed batch")
    for x in (c, p, f16):
        lib.qmha_kv_cache_destroy(x)


@pytest.mark.parametrize("G", [1, 2, 4, 8])
def test_grid_bounds_cover_every_sequence(G):
    """PB = ceil((total / 32 + 2 B) G / 4) + B and the append's total / 32 + 2 B against the true counts: a sequence of nq rows
    ending at L has Ga = ceil32((L - nq) % 32 + nq) / 32 query groups and ceil(Ga G / 4) unit blocks; n rows at p touch
    (p + n - 1) / 32 - p / 32 + 1 groups.  Per sequence the worst L / p is taken, then every pair of sequences is summed."""
    blocks = {nq: max(-(-((((L - nq) % 32 + nq + 31) // 32) * G) // 4) for L in range(nq, nq + 32)) for nq in range(1, 100)}
    groups = {n: max((p + n - 1) // 32 - p // 32 + 1 for p in range(32)) for n in range(1, 100)}
    for n0 in range(1, 100):
        for n1 in range(1, 100):
            total, B = n0 + n1, 2
            assert blocks[n0] + blocks[n1] <= -(-((total // 32 + 2 * B) * G) // 4) + B, (n0, n1)
            assert groups[n0] + groups[n1] <= total // 32 + 2 * B, (n0, n1)
