"""CPU tests of the fp8 cache's shared-prefix decode call: the interface in the header, the library and the
bindings, and the host refusals (every host check runs before any HIP call, so dummy pointers reach them)."""
import ctypes
import os
import re

import pytest

from tests.test_fp8_cpu import CAUSAL, DUMMY, FP8, MEM, V1A, lib, make  # noqa: F401

NAMES = ("qmha_attend_cached_decode_shared", "qmha_attend_cached_paged_decode_shared")


def test_signatures(lib):
    from quantizedmha_amd import _lib, torch_ext
    i, vp, sz = ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t
    assert _lib.SIGNATURES[NAMES[0]] == (i, [vp, vp, vp, i, vp, i, i, vp, sz, ctypes.c_uint, vp])
    assert _lib.SIGNATURES[NAMES[1]] == (i, [vp, vp, vp, i, vp, vp, i, i, vp, sz, ctypes.c_uint, vp])
    with open(os.path.join(os.path.dirname(_lib.__file__), "..", "include", "launchers.h")) as f:
        header = f.read()
    for name in NAMES:
        assert re.search(rf"\bint {name}\(", header) and getattr(lib, name).restype is i
    for cls, method in ((torch_ext.KVCache, "attend_decode_shared"), (torch_ext.GroupedKVCache, "attend_decode_shared"),
                        (torch_ext.PagedKVCache, "attend_paged_decode_shared")):
        assert callable(getattr(cls, method))


@pytest.mark.parametrize("paged", [False, True])
def test_host_refusals(lib, paged):
    c, other, f16 = make(lib, paged=paged), make(lib, paged=not paged), make(lib, V1A, paged=paged)  # B 2, cap 256, h 2, d 64
    big, what = 1 << 30, "attend_paged_decode_shared" if paged else "attend_decode_shared"
    fn = getattr(lib, NAMES[paged])

    def call(cache=c, nq=1, lens=DUMMY, table=DUMMY, prefix=128, chunk=64, scratch=MEM, nbytes=big, flags=CAUSAL):
        return fn(cache, DUMMY, DUMMY, nq, lens, *([table] if paged else []), prefix, chunk, scratch, nbytes, flags, None)

    def refused(st, status, *words):
        msg = lib.qmha_last_error().decode()
        assert st == status and what in msg and all(w in msg for w in words), (st, msg)

    for prefix in (0, 63, 96, 256 + 64):  # 0, chunk_rows - 1, no multiple of chunk_rows, cap + chunk_rows
        refused(call(prefix=prefix), 1, f"prefix_rows = {prefix} ", "multiple of chunk_rows = 64", "= 256", "attend_decode")
    refused(call(prefix=64, chunk=128), 1, "prefix_rows = 64 ", "chunk_rows = 128", "attend_decode")
    refused(call(nq=33), 1, "Nq * (h / h_kv) = 33 * 1 = 33", "limit is 32")
    refused(call(lens=None), 1, "null lens")
    if paged:
        refused(call(table=None), 1, "null table")
    refused(call(scratch=None), 1, "null scratch", "qmha_attend_decode_bytes")
    need = lib.qmha_attend_decode_bytes(c, 1, 64)
    refused(call(nbytes=need - 1), 1, "scratch too small", str(need))
    refused(call(flags=0), 1, "QMHA_FLAG_CAUSAL")
    refused(call(cache=other), 1, "the cache is contiguous" if paged else "the cache is paged")
    refused(call(cache=f16), 4, "fa_tc_v1a", "attend_tokens_split")
    for x in (c, other, f16):
        lib.qmha_kv_cache_destroy(x)
