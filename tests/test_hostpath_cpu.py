"""CPU tests of the host path's check order: which error wins when a call is wrong in two ways.

Every solve entry point goes through one checked path, whose order is: shape with Nq, shape with Nk, h_kv, flag bits,
causal Nq > Nk, "not built" for the kind of call (grouped-query before rectangular before causal), "workspace too
small".  The cache entry points check their arguments in the order of their parameters' first use.  All of it runs
before any HIP call, so every case is reached with dummy pointers (as tests/test_gqa_cpu.py does).  Each case asserts
the status and a fragment of the winning message; the loser's fragment must be absent.
"""
import ctypes

import pytest

CAUSAL = 1
INVALID, NOSYS = 1, 4
FA, V1A, INT8, UNFUSED = 0, 1, 2, 3
MEM = 0x10000  # 256-byte aligned, never dereferenced: checks run first
DUMMY = ctypes.c_void_p(0x1000)


@pytest.fixture(scope="module")
def lib():
    from tools.build import build
    build(verbose=False)
    from quantizedmha_amd import _lib
    return _lib.load()


def solve_gqa(lib, B=2, Nq=64, Nk=128, d_model=256, h=4, h_kv=2, vid=INT8, flags=0, ws=None, ws_bytes=0):
    st = lib.qmha_solve_gqa(DUMMY, DUMMY, DUMMY, DUMMY, B, Nq, Nk, d_model, h, h_kv, vid, flags, ws, ws_bytes, None)
    return st, lib.qmha_last_error().decode()


def create_gqa(lib, B=2, cap=256, d_model=256, h=4, h_kv=4, vid=INT8, mem=MEM, nbytes=1 << 30):
    handle = ctypes.c_void_p()
    st = lib.qmha_kv_cache_create_gqa(ctypes.byref(handle), ctypes.c_void_p(mem), nbytes, B, cap, d_model, h, h_kv, vid)
    return st, lib.qmha_last_error().decode(), handle


# (arguments wrong in two ways, status, the winner's fragment, the loser's fragment); h_kv is added by the test
TWO_FAULTS = [
    (dict(Nk=100, flags=2), INVALID, "Nk must be a multiple of 32", "flag bits"),
    (dict(Nq=128, Nk=64, flags=2 | CAUSAL), INVALID, "unknown flag bits 2", "bottom-right"),
    (dict(Nq=128, Nk=64, flags=CAUSAL, vid=FA), INVALID, "needs Nk >= Nq (Nq = 128, Nk = 64)", "not built"),
    (dict(Nq=64, Nk=128, vid=UNFUSED, ws=DUMMY, ws_bytes=1), NOSYS, "is not built for variant unfused at d = 64", "too small"),
    (dict(Nq=64, Nk=128, d_model=128, vid=V1A, ws=DUMMY, ws_bytes=1), NOSYS, "is not built for variant fa_tc_v1a at d = 32",
     "too small"),
    (dict(Nq=48, vid=99), INVALID, "Nq must be a multiple of 32", "unknown variant"),
]


@pytest.mark.parametrize("h_kv", [4, 2])  # h_kv == h and h_kv < h
@pytest.mark.parametrize("kw,status,winner,loser", TWO_FAULTS)
def test_first_failure_of_a_solve(lib, h_kv, kw, status, winner, loser):
    st, msg = solve_gqa(lib, h_kv=h_kv, **kw)
    assert st == status and winner in msg and loser not in msg, (st, msg)


@pytest.mark.parametrize("h_kv", [0, 3])
def test_bad_row_count_wins_over_bad_kv_heads(lib, h_kv):
    st, msg = solve_gqa(lib, Nq=48, h_kv=h_kv)
    assert st == INVALID and "Nq must be a multiple of 32" in msg and "h_kv" not in msg, (st, msg)


# the kind of call names the feature: (h_kv, Nq, Nk, flags) -> fragment; the other two fragments must be absent
FEATURES = ("causal attention is not built", "rectangular attention (Nq != Nk) is not built",
            "grouped-query attention (h_kv < h) is not built")
KINDS = [
    (4, 128, 128, CAUSAL, 0),
    (4, 64, 128, 0, 1),
    (4, 64, 128, CAUSAL, 1),
    (2, 64, 128, 0, 2),
    (2, 64, 128, CAUSAL, 2),
    (2, 128, 128, 0, 2),
    (2, 128, 128, CAUSAL, 2),
]


@pytest.mark.parametrize("vid,name,d_model", [(FA, "fa", 256), (V1A, "fa_tc_v1a", 128)])  # h = 4: fa at d = 64, fp16 at d = 32
@pytest.mark.parametrize("h_kv,Nq,Nk,flags,kind", KINDS)
def test_the_kind_of_call_names_the_unbuilt_feature(lib, vid, name, d_model, h_kv, Nq, Nk, flags, kind):
    st, msg = solve_gqa(lib, Nq=Nq, Nk=Nk, d_model=d_model, h_kv=h_kv, vid=vid, flags=flags)
    assert st == NOSYS and msg.startswith(FEATURES[kind] + " for variant " + name + " at d = " + str(d_model // 4)), (st, msg)
    assert msg.endswith("(fa_tc_v1a: d = 64, 128; fa_tc_int8_b: d = 32, 64, 128)"), msg


@pytest.mark.parametrize("h_kv,feature", [(4, "the persistent K/V cache is not built"),
                                          (2, "grouped-query attention (h_kv < h) is not built")])
def test_create_names_the_unbuilt_feature(lib, h_kv, feature):
    st, msg, handle = create_gqa(lib, h_kv=h_kv, vid=FA)
    assert st == NOSYS and msg.startswith(feature + " for variant fa at d = 64") and not handle.value, (st, msg)


def test_create_misaligned_memory_wins_over_too_few_bytes(lib):
    st, msg, handle = create_gqa(lib, mem=MEM + 16, nbytes=1)
    assert st == INVALID and "256-byte aligned" in msg and "too small" not in msg and not handle.value, (st, msg)


@pytest.fixture
def cache(lib):
    st, msg, handle = create_gqa(lib)
    assert st == 0, msg
    yield handle
    lib.qmha_kv_cache_destroy(handle)


def test_attend_bad_row_count_wins_over_unknown_flags(lib, cache):
    st = lib.qmha_attend_cached(cache, DUMMY, DUMMY, 48, 2, None)
    msg = lib.qmha_last_error().decode()
    assert st == INVALID and "Nq must be a multiple of 32" in msg and "flag bits" not in msg, (st, msg)


def test_attend_varlen_unknown_flags_win_over_null_lens(lib, cache):
    st = lib.qmha_attend_cached_varlen(cache, DUMMY, DUMMY, 32, None, 2, None)
    msg = lib.qmha_last_error().decode()
    assert st == INVALID and "unknown flag bits 2" in msg and "lens" not in msg, (st, msg)


@pytest.fixture
def paged(lib):
    handle = ctypes.c_void_p()  # 12 pages of 64 rows, 5 per sequence: cap = 320
    st = lib.qmha_kv_cache_create_paged(ctypes.byref(handle), ctypes.c_void_p(MEM), 1 << 30, 2, 12, 64, 5, 256, 4, 2, INT8)
    assert st == 0, lib.qmha_last_error()
    yield handle
    lib.qmha_kv_cache_destroy(handle)


# The uniform-count token-granular entry points, wrong in two ways: (entry point, which cache, the
# arguments behind the handle, the winner's fragment, the loser's fragment).  Neither int8 cache has its tail attached.
TOKEN_FAULTS = [
    ("qmha_kv_cache_append_tokens", "paged", (None, DUMMY, 3, DUMMY, None), "append_tokens: the cache is paged", "null tensor"),
    ("qmha_kv_cache_append_tokens", "cache", (None, DUMMY, 3, None, None), "null tensor pointer", "pos"),
    ("qmha_kv_cache_append_tokens", "cache", (DUMMY, DUMMY, 257, None, None), "append_tokens: null pos (a device int32[B])", "rows"),
    ("qmha_kv_cache_append_tokens", "cache", (DUMMY, DUMMY, 0, DUMMY, None), "append_tokens: n = 0 rows, needs 1 <= n <= cap = 256",
     "tail"),
    ("qmha_kv_cache_append_tokens", "cache", (DUMMY, DUMMY, 256, DUMMY, None), "append_tokens: an int8 cache needs its tail", "rows"),
    ("qmha_attend_cached_tokens", "paged", (DUMMY, DUMMY, 3, None, CAUSAL, None), "attend_tokens: the cache is paged", "lens"),
    ("qmha_attend_cached_tokens", "cache", (DUMMY, None, 3, None, CAUSAL, None), "null tensor pointer", "lens"),
    ("qmha_attend_cached_tokens", "cache", (DUMMY, DUMMY, 3, None, 0, None), "attend_tokens: null lens (a device int32[B])", "flags"),
    ("qmha_attend_cached_tokens", "cache", (DUMMY, DUMMY, 257, DUMMY, 0, None), "attend_tokens: flags must be QMHA_FLAG_CAUSAL",
     "rows"),
    ("qmha_attend_cached_tokens", "cache", (DUMMY, DUMMY, 0, DUMMY, CAUSAL, None),
     "attend_tokens: Nq = 0 rows, needs 1 <= Nq <= cap = 256", "flags"),
    ("qmha_kv_cache_append_paged", "cache", (DUMMY, DUMMY, 3, None, DUMMY, None), "append_paged: the cache is contiguous", "pos"),
    ("qmha_kv_cache_append_paged", "paged", (DUMMY, None, 3, None, DUMMY, None), "null tensor pointer", "pos"),
    ("qmha_kv_cache_append_paged", "paged", (DUMMY, DUMMY, 3, None, None, None), "append_paged: null pos (a device int32[B])", "table"),
    ("qmha_kv_cache_append_paged", "paged", (DUMMY, DUMMY, 321, DUMMY, None, None),
     "append_paged: null table (a device int32[B][max_pages])", "rows"),
    ("qmha_kv_cache_append_paged", "paged", (DUMMY, DUMMY, 321, DUMMY, DUMMY, None),
     "append_paged: n = 321 rows, needs 1 <= n <= cap = max_pages * page_rows = 320", "tail"),
    ("qmha_kv_cache_append_paged", "paged", (DUMMY, DUMMY, 320, DUMMY, DUMMY, None), "append_paged: an int8 cache needs its tail", "rows"),
    ("qmha_attend_cached_paged", "cache", (DUMMY, DUMMY, 3, None, DUMMY, CAUSAL, None), "attend_paged: the cache is contiguous", "lens"),
    ("qmha_attend_cached_paged", "paged", (None, DUMMY, 3, None, DUMMY, CAUSAL, None), "null tensor pointer", "lens"),
    ("qmha_attend_cached_paged", "paged", (DUMMY, DUMMY, 3, None, None, CAUSAL, None), "attend_paged: null lens (a device int32[B])",
     "table"),
    ("qmha_attend_cached_paged", "paged", (DUMMY, DUMMY, 3, DUMMY, None, 0, None),
     "attend_paged: null table (a device int32[B][max_pages])", "flags"),
    ("qmha_attend_cached_paged", "paged", (DUMMY, DUMMY, 321, DUMMY, DUMMY, 3, None), "attend_paged: flags must be QMHA_FLAG_CAUSAL",
     "rows"),
    ("qmha_attend_cached_paged", "paged", (DUMMY, DUMMY, 321, DUMMY, DUMMY, CAUSAL, None),
     "attend_paged: Nq = 321 rows, needs 1 <= Nq <= cap = max_pages * page_rows = 320", "flags"),
]


@pytest.mark.parametrize("entry,which,args,winner,loser", TOKEN_FAULTS)
def test_first_failure_of_a_token_granular_call(lib, cache, paged, entry, which, args, winner, loser):
    st = getattr(lib, entry)({"cache": cache, "paged": paged}[which], *args)
    msg = lib.qmha_last_error().decode()
    assert st == INVALID and winner in msg and loser not in msg, (st, msg)


@pytest.mark.parametrize("entry,args", [("qmha_kv_cache_append_tokens", (DUMMY, DUMMY, 0, None, None)),
                                        ("qmha_attend_cached_tokens", (DUMMY, DUMMY, 0, None, 0, None)),
                                        ("qmha_kv_cache_append_paged", (DUMMY, DUMMY, 0, None, None, None)),
                                        ("qmha_attend_cached_paged", (DUMMY, DUMMY, 0, None, None, 0, None))])
def test_a_null_cache_wins_over_everything_else(lib, entry, args):
    st = getattr(lib, entry)(None, *args)
    assert st == INVALID and lib.qmha_last_error().decode() == "null cache", (st, lib.qmha_last_error())


def test_solve_ws_null_workspace_holds_no_bytes(lib):
    st = lib.qmha_solve_ws(DUMMY, DUMMY, DUMMY, DUMMY, 2, 64, 256, 4, INT8, None, 1 << 30, None)
    assert st == INVALID and lib.qmha_last_error().decode() == "workspace too small", (st, lib.qmha_last_error())
