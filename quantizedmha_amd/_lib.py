"""ctypes binding of the native C-ABI (include/launchers.h) -- the only way the Python
layer reaches the HIP kernels.  There is no fallback: if libqmha.so is missing or fails to
load, every entry point raises, so a GPU run can never silently take another path."""
from __future__ import annotations

import ctypes
import os
import threading

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_DIR = os.path.join(HERE, "lib")
# QMHA_LIB_PATH: load another build of the same C-ABI (A/B kernel experiments); still no fallback
LIB_PATH = os.environ.get("QMHA_LIB_PATH") or os.path.join(LIB_DIR, "libqmha.so")

VARIANTS = {"fa": 0, "fa_tc_v1a": 1, "fa_tc_int8_b": 2, "unfused": 3, "fa_mfma": 4, "fa_tc_int8_pt": 5}
DEFAULT_KERNEL = "fa_tc_int8_b"
QMHA_OK = 0
QMHA_FLAG_CAUSAL = 1  # qmha_solve_opts: query row r attends keys j <= r

# every symbol include/launchers.h declares, with its ctypes signature
_i, _sz, _vp, _cp = ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_char_p
SIGNATURES = {
    "solve": (None, [_vp, _vp, _vp, _vp, _i, _i, _i]),
    "qmha_solve_ex": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "qmha_solve_opts": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, ctypes.c_uint, _vp, _sz, _vp]),
    "qmha_solve_rect": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, ctypes.c_uint, _vp, _sz, _vp]),
    "qmha_solve_gqa": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, ctypes.c_uint, _vp, _sz, _vp]),
    "qmha_workspace_size": (_sz, [_i, _i, _i, _i, _i]),
    # persistent K/V cache: the handle is an opaque pointer
    "qmha_kv_cache_bytes": (_sz, [_i, _i, _i, _i, _i]),
    "qmha_kv_cache_create": (_i, [ctypes.POINTER(_vp), _vp, _sz, _i, _i, _i, _i, _i]),
    "qmha_kv_cache_create_gqa": (_i, [ctypes.POINTER(_vp), _vp, _sz, _i, _i, _i, _i, _i, _i]),
    "qmha_kv_cache_destroy": (None, [_vp]),
    "qmha_kv_cache_len": (_i, [_vp]),
    "qmha_kv_cache_truncate": (_i, [_vp, _i]),
    "qmha_kv_cache_append": (_i, [_vp, _vp, _vp, _i, _vp]),
    "qmha_attend_cached": (_i, [_vp, _vp, _vp, _i, ctypes.c_uint, _vp]),
    # per-sequence rows / lengths: device int32[B] pointers
    "qmha_kv_cache_append_at": (_i, [_vp, _vp, _vp, _i, _vp, _vp]),
    "qmha_attend_cached_varlen": (_i, [_vp, _vp, _vp, _i, _vp, ctypes.c_uint, _vp]),
    # token-granular lengths: the int8 cache's tail of raw rows, and append / attend at any length
    "qmha_kv_cache_tail_bytes": (_sz, [_vp]),
    "qmha_kv_cache_attach_tail": (_i, [_vp, _vp, _sz]),
    "qmha_kv_cache_append_tokens": (_i, [_vp, _vp, _vp, _i, _vp, _vp]),
    "qmha_attend_cached_tokens": (_i, [_vp, _vp, _vp, _i, _vp, ctypes.c_uint, _vp]),
    # paged caches: a pool of pages, and a device int32[B][max_pages] block table beside pos / lens
    "qmha_kv_cache_paged_bytes": (_sz, [_i, _i, _i, _i, _i, _i]),
    "qmha_kv_cache_create_paged": (_i, [ctypes.POINTER(_vp), _vp, _sz, _i, _i, _i, _i, _i, _i, _i, _i]),
    "qmha_kv_cache_append_paged": (_i, [_vp, _vp, _vp, _i, _vp, _vp, _vp]),
    "qmha_attend_cached_paged": (_i, [_vp, _vp, _vp, _i, _vp, _vp, ctypes.c_uint, _vp]),
    # split-KV: the two attends with the key sweep in chunks, over the caller's scratch
    "qmha_attend_split_bytes": (_sz, [_vp, _i, _i]),
    "qmha_attend_cached_tokens_split": (_i, [_vp, _vp, _vp, _i, _vp, _i, _vp, _sz, ctypes.c_uint, _vp]),
    "qmha_attend_cached_paged_split": (_i, [_vp, _vp, _vp, _i, _vp, _vp, _i, _vp, _sz, ctypes.c_uint, _vp]),
    # a sliding window: the two attends over the last `window` keys of a row (a host int, a multiple of 32)
    "qmha_attend_cached_tokens_window": (_i, [_vp, _vp, _vp, _i, _vp, _i, ctypes.c_uint, _vp]),
    "qmha_attend_cached_paged_window": (_i, [_vp, _vp, _vp, _i, _vp, _vp, _i, ctypes.c_uint, _vp]),
    # packed batches: operands without a batch axis and a device int32[B + 1] cu beside pos / lens / table
    "qmha_kv_cache_append_packed": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp, _vp]),
    "qmha_kv_cache_append_paged_packed": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp]),
    "qmha_attend_cached_packed": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp, ctypes.c_uint, _vp]),
    "qmha_attend_cached_paged_packed": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp, _vp, ctypes.c_uint, _vp]),
    "qmha_solve_ws": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _sz, _vp]),
    "qmha_solve_variant": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i]),
    "qmha_quantize_int8": (_i, [_vp, _i, _i, _i, _i, _vp, _vp, _i, _vp]),
    "qmha_debug_qk_int32": (_i, [_vp, _vp, _i, _i, _i, _i, _vp]),
    "qmha_debug_fa_int8_dump": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp]),
    "qmha_debug_fa_int8_pt_dump": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp]),
    "qmha_debug_fa_int8_pstage": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, ctypes.c_uint] + [_vp] * 8),
    "qmha_variant_from_name": (_i, [_cp]),
    "qmha_variant_name": (_cp, [_i]),
    "qmha_status_string": (_cp, [_i]),
    "qmha_version": (_cp, []),
    "qmha_last_error": (_cp, []),
    "qmha_profile_enable": (None, [_i]),
    "qmha_set_overlap_chunks": (_i, [_i]),
    "qmha_debug_set_pt_wait": (ctypes.c_longlong, [ctypes.c_longlong]),
    "qmha_profile_collect": (_i, [ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_longlong),
                                  ctypes.POINTER(ctypes.c_double)]),
    "qmha_release_workspaces": (None, []),
}

_lock = threading.Lock()
_lib = None


class QMHAError(RuntimeError):
    pass


def load(path: str = LIB_PATH):
    """Load libqmha.so (built by tools/build.py / __graft_entry__.build())."""
    global _lib
    with _lock:
        if _lib is None:
            if not os.path.exists(path):
                raise QMHAError(f"native library {path} not found: run `python tools/build.py` "
                                "(quantizedmha_amd has no non-HIP fallback)")
            lib = ctypes.CDLL(path)
            for name, (res, args) in SIGNATURES.items():
                fn = getattr(lib, name)
                fn.restype = res
                fn.argtypes = args
            _lib = lib
    return _lib


def check(status: int, what: str = "qmha") -> None:
    if status != QMHA_OK:
        lib = load()
        raise QMHAError(f"{what}: {lib.qmha_status_string(status).decode()}: {lib.qmha_last_error().decode()}")


def variant_id(kernel: str) -> int:
    if kernel not in VARIANTS:
        raise KeyError(kernel)
    return VARIANTS[kernel]
