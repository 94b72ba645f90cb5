"""CPU tests of the persistent K/V cache: qmha_kv_cache_* and qmha_attend_cached.

Every check of the new entry points runs before any HIP call, so they are reached here with dummy pointers (as
tests/test_rect_cpu.py does for qmha_solve_rect); an append that passes them fails at the launch on a machine without
a GPU and must leave the cache's length where it was.  The shipped library holds the five append kernels and still
ten masked main kernels: the cached call launches the rectangular instances, it adds none.
"""
import ctypes
import os
import re
import subprocess

import pytest

from tests import append_syms

from tests import gpu_support as gs
from tests.gpu_support import CAUSAL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V1A, INT8 = 1, 2  # the C-ABI's variant ids, not gpu_support's names
MEM = 0x10000  # 256-byte aligned, never dereferenced: checks run first
BUILT = [({gs.INT8: INT8, gs.F16: V1A}[v], d) for v, d in gs.BUILT]


@pytest.fixture(scope="module")
def lib():
    from tools.build import build
    build(verbose=False)
    from quantizedmha_amd import _lib
    return _lib.load()


def create(lib, B, cap, d_model, h, vid, mem=MEM, nbytes=None):
    """(status, message, handle); nbytes defaults to qmha_kv_cache_bytes."""
    if nbytes is None:
        nbytes = lib.qmha_kv_cache_bytes(B, cap, d_model, h, vid)
    handle = ctypes.c_void_p()
    st = lib.qmha_kv_cache_create(ctypes.byref(handle), ctypes.c_void_p(mem) if mem else None, nbytes, B, cap, d_model, h, vid)
    return st, lib.qmha_last_error().decode(), handle


@pytest.fixture
def cache(lib):
    st, msg, handle = create(lib, 2, 256, 128, 2, INT8)
    assert st == 0 and handle.value, (st, msg)
    yield handle
    lib.qmha_kv_cache_destroy(handle)


def has_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except ImportError:
        return False


@pytest.mark.parametrize("vid,d", BUILT)
def test_cache_bytes_is_the_workspace_at_cap(lib, vid, d):
    for B, cap, h in ((2, 256, 2), (16, 4096, 16)):
        need = lib.qmha_kv_cache_bytes(B, cap, h * d, h, vid)
        assert need == lib.qmha_workspace_size(B, cap, h * d, h, vid) > 0


@pytest.mark.parametrize("shape", [(1, 32, 32, 1, INT8), (3, 1024, 256, 4, V1A)])
def test_cache_bytes_other_shapes(lib, shape):
    assert lib.qmha_kv_cache_bytes(*shape) == lib.qmha_workspace_size(*shape) > 0


@pytest.mark.parametrize("vid,d", BUILT)
def test_create_starts_empty(lib, vid, d):
    st, msg, handle = create(lib, 2, 96, 2 * d, 2, vid)
    assert st == 0 and handle.value, (st, msg)
    assert lib.qmha_kv_cache_len(handle) == 0
    lib.qmha_kv_cache_destroy(handle)


@pytest.mark.parametrize("vid,name,d_model,h", [
    (0, "fa", 128, 2), (3, "unfused", 128, 2), (4, "fa_mfma", 128, 2), (5, "fa_tc_int8_pt", 128, 2),
    (INT8, "fa_tc_int8_b", 192, 2),  # d = 96
    (V1A, "fa_tc_v1a", 64, 2),       # d = 32: int8 only
])
def test_create_unsupported_combinations_are_nosys(lib, vid, name, d_model, h):
    st, msg, handle = create(lib, 1, 128, d_model, h, vid, nbytes=1 << 30)
    assert st == 4 and not handle.value, (st, msg)
    assert name in msg and f"d = {d_model // h}" in msg and "cache" in msg, msg


@pytest.mark.parametrize("kw,cause", [
    (dict(cap=100), "cap must be a multiple of 32"),
    (dict(cap=0), "positive"),
    (dict(mem=MEM + 16), "256-byte aligned"),
    (dict(mem=0), "null"),
    (dict(short=1), "too small"),
    (dict(h=3), "divisible"),
    (dict(vid=7), "unknown variant"),
])
def test_create_invalid_arguments(lib, kw, cause):
    a = dict(B=2, cap=256, d_model=128, h=2, vid=INT8, mem=MEM, short=0)
    a.update(kw)
    nbytes = lib.qmha_kv_cache_bytes(2, 256, 128, 2, INT8) - a["short"]
    st, msg, handle = create(lib, a["B"], a["cap"], a["d_model"], a["h"], a["vid"], a["mem"], nbytes)
    assert st == 1 and cause in msg and not handle.value, (st, msg)


def test_append_rejections_leave_the_length(lib, cache):
    dummy = ctypes.c_void_p(0x1000)
    for n, cause in ((48, "multiple of 32"), (0, "multiple of 32"), (-32, "multiple of 32"), (288, "exceed cap")):
        st = lib.qmha_kv_cache_append(cache, dummy, dummy, n, None)
        assert st == 1 and cause in lib.qmha_last_error().decode(), (n, st, lib.qmha_last_error())
        assert lib.qmha_kv_cache_len(cache) == 0
    assert lib.qmha_kv_cache_append(cache, None, dummy, 32, None) == 1 and "null" in lib.qmha_last_error().decode()
    assert lib.qmha_kv_cache_len(cache) == 0


def test_attend_rejections(lib, cache):
    dummy = ctypes.c_void_p(0x1000)
    for Nq, flags, cause in ((32, CAUSAL, "len >= Nq"),            # nothing appended yet
                             (32, 0, "no unmasked mode"),          # len < cap without the mask
                             (32, 2, "flag"), (32, 0x80000001, "flag"),
                             (40, CAUSAL, "Nq must be a multiple of 32"), (0, CAUSAL, "positive")):
        st = lib.qmha_attend_cached(cache, dummy, dummy, Nq, flags, None)
        assert st == 1 and cause in lib.qmha_last_error().decode(), (Nq, flags, st, lib.qmha_last_error())
    assert lib.qmha_attend_cached(cache, None, dummy, 32, CAUSAL, None) == 1 and "null" in lib.qmha_last_error().decode()


def test_truncate_rules(lib, cache):
    assert lib.qmha_kv_cache_truncate(cache, 32) == 1 and "above" in lib.qmha_last_error().decode()  # upward
    assert lib.qmha_kv_cache_truncate(cache, -32) == 1
    assert lib.qmha_kv_cache_truncate(cache, 16) == 1 and "multiple of 32" in lib.qmha_last_error().decode()
    assert lib.qmha_kv_cache_truncate(cache, 0) == 0 and lib.qmha_kv_cache_len(cache) == 0


@pytest.mark.skipif(has_gpu(), reason="needs a machine without a GPU: the launch itself must fail")
def test_failed_launch_leaves_the_length(lib, cache):
    """A valid append reaches the launch, which fails without a device: QMHA_ERR_HIP and len stays 0, with and without
    profiling (whose first event cannot be created either)."""
    dummy = ctypes.c_void_p(0x1000)
    assert lib.qmha_kv_cache_append(cache, dummy, dummy, 64, None) == 2, lib.qmha_last_error()
    assert lib.qmha_kv_cache_len(cache) == 0
    lib.qmha_profile_enable(1)
    try:
        assert lib.qmha_kv_cache_append(cache, dummy, dummy, 64, None) == 2
    finally:
        lib.qmha_profile_enable(0)
    assert lib.qmha_kv_cache_len(cache) == 0
    assert lib.qmha_attend_cached(cache, dummy, dummy, 32, CAUSAL, None) == 1  # still empty


def test_library_has_five_append_kernels_and_ten_masked(lib):
    path = os.path.join(ROOT, "quantizedmha_amd", "lib", "libqmha.so")
    syms = subprocess.run(["nm", path], capture_output=True, text=True, check=True).stdout
    # the append template over HostRow (its other row policy: test_varlen_cpu.py)
    stubs = append_syms.append(syms, row="HostRow")
    assert stubs == [("qmha_kv_append_f16_kernel", "HostRow", "128"), ("qmha_kv_append_f16_kernel", "HostRow", "64"),
                     ("qmha_kv_append_int8_kernel", "HostRow", "128"), ("qmha_kv_append_int8_kernel", "HostRow", "32"),
                     ("qmha_kv_append_int8_kernel", "HostRow", "64")], stubs
    append_syms.check_family(syms)
    masked = set(re.findall(r"__device_stub__(qmha_fa_\w+?_masked_kernel)ILi(\d+)ENS_\d+([A-Za-z]+?)E(\w*)", syms))
    # the cache runs the shipped Rect instances: still ten of the SquareCausal and Rect geometries, and beside them
    # nothing but the five grouped-query ones
    assert len([m for m in masked if m[2] in ("SquareCausal", "Rect")]) == 10, sorted(masked)
    assert len(masked) == 15 and {m[2] for m in masked} == {"SquareCausal", "Rect", "Grouped"}, sorted(masked)


def test_python_binding_has_kvcache():
    import inspect
    from quantizedmha_amd import torch_ext
    sig = inspect.signature(torch_ext.KVCache.__init__)
    assert list(sig.parameters) == ["self", "B", "cap", "d_model", "num_heads", "kernel", "device"]
    assert sig.parameters["kernel"].default == "fa_tc_int8_b"
    for name in ("append", "attend", "truncate", "len"):
        assert hasattr(torch_ext.KVCache, name), name
    assert inspect.signature(torch_ext.KVCache.attend).parameters["causal"].default is True


def test_compiled_module_has_kvcache(lib):
    import sys
    from quantizedmha_amd import _lib
    sys.path.insert(0, _lib.LIB_DIR)
    try:
        import torch_ext
    finally:
        sys.path.pop(0)
    assert "append" in dir(torch_ext.KVCache) and "attend" in dir(torch_ext.KVCache) and "truncate" in dir(torch_ext.KVCache)
    assert "kernel: str = 'fa_tc_int8_b'" in torch_ext.KVCache.__init__.__doc__
