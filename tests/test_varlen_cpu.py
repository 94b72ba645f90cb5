"""CPU tests of the per-sequence entry points of the K/V cache: qmha_kv_cache_append_at and
qmha_attend_cached_varlen.

Every host check of the two calls runs before any HIP call, so they are reached here with dummy pointers (as
tests/test_kvcache_cpu.py does); neither call reads or changes the cache's host length.  The shipped library holds
five varlen main kernels and five placement kernels under names of their own, beside the fifteen masked and the five
append kernels it held before.
"""
import ctypes
import inspect
import os
import re
import subprocess

import pytest

from tests import append_syms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAUSAL = 1
V1A, INT8 = 1, 2
MEM = 0x10000  # 256-byte aligned, never dereferenced: checks run first
DUMMY = ctypes.c_void_p(0x1000)


@pytest.fixture(scope="module")
def lib():
    from tools.build import build
    build(verbose=False)
    from quantizedmha_amd import _lib
    return _lib.load()


@pytest.fixture(params=["multi-head", "grouped"])
def cache(lib, request):
    """B = 2, cap = 256, h = 2 (grouped: h = 4 on 2 K/V heads), d = 64, int8."""
    handle = ctypes.c_void_p()
    if request.param == "multi-head":
        nbytes = lib.qmha_kv_cache_bytes(2, 256, 128, 2, INT8)
        st = lib.qmha_kv_cache_create(ctypes.byref(handle), ctypes.c_void_p(MEM), nbytes, 2, 256, 128, 2, INT8)
    else:
        nbytes = lib.qmha_kv_cache_bytes(2, 256, 128, 2, INT8)
        st = lib.qmha_kv_cache_create_gqa(ctypes.byref(handle), ctypes.c_void_p(MEM), nbytes, 2, 256, 256, 4, 2, INT8)
    assert st == 0 and handle.value, (st, lib.qmha_last_error())
    yield handle
    lib.qmha_kv_cache_destroy(handle)


def test_header_declares_the_two_calls():
    header = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "launchers.h")).read())
    assert ("int qmha_kv_cache_append_at(qmha_kv_cache_t *c, const float *K, const float *V, int n, const int32_t *pos, "
            "void *stream);") in header
    assert ("int qmha_attend_cached_varlen(qmha_kv_cache_t *c, const float *Q, float *O, int Nq, const int32_t *lens, "
            "unsigned flags, void *stream);") in header


def test_library_exports_the_two_calls(lib):
    from quantizedmha_amd import _lib
    vp, i = ctypes.c_void_p, ctypes.c_int
    for name, argtypes in (("qmha_kv_cache_append_at", [vp, vp, vp, i, vp, vp]),
                           ("qmha_attend_cached_varlen", [vp, vp, vp, i, vp, ctypes.c_uint, vp])):
        fn = getattr(lib, name)  # AttributeError on a library without the symbol
        assert fn.restype is i and list(fn.argtypes) == argtypes, name
    path = os.path.join(_lib.LIB_DIR, "libqmha.so")
    dyn = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    assert re.search(r" T qmha_kv_cache_append_at$", dyn, re.M) and re.search(r" T qmha_attend_cached_varlen$", dyn, re.M)


def test_append_at_rejections_leave_the_length(lib, cache):
    for n, cause in ((48, "multiple of 32"), (0, "multiple of 32"), (-32, "multiple of 32"), (288, "exceed cap")):
        st = lib.qmha_kv_cache_append_at(cache, DUMMY, DUMMY, n, DUMMY, None)
        assert st == 1 and cause in lib.qmha_last_error().decode(), (n, st, lib.qmha_last_error())
        assert lib.qmha_kv_cache_len(cache) == 0
    for args, cause in (((None, DUMMY, 32, DUMMY), "null tensor"), ((DUMMY, None, 32, DUMMY), "null tensor"),
                        ((DUMMY, DUMMY, 32, None), "null pos")):
        assert lib.qmha_kv_cache_append_at(cache, *args, None) == 1 and cause in lib.qmha_last_error().decode(), args
        assert lib.qmha_kv_cache_len(cache) == 0
    assert lib.qmha_kv_cache_append_at(None, DUMMY, DUMMY, 32, DUMMY, None) == 1 and "null cache" in lib.qmha_last_error().decode()


def test_attend_varlen_rejections_leave_the_length(lib, cache):
    for Nq, flags, cause in ((32, 2, "flag"), (32, 0x80000001, "flag"), (40, CAUSAL, "Nq must be a multiple of 32"),
                             (40, 0, "Nq must be a multiple of 32"), (0, CAUSAL, "positive"), (-32, 0, "positive"),
                             (288, CAUSAL, "Nq <= cap")):  # causal: Nq rows cannot be the last rows of fewer
        st = lib.qmha_attend_cached_varlen(cache, DUMMY, DUMMY, Nq, DUMMY, flags, None)
        assert st == 1 and cause in lib.qmha_last_error().decode(), (Nq, flags, st, lib.qmha_last_error())
        assert lib.qmha_kv_cache_len(cache) == 0
    for args, cause in (((None, DUMMY, 32, DUMMY), "null tensor"), ((DUMMY, None, 32, DUMMY), "null tensor"),
                        ((DUMMY, DUMMY, 32, None), "null lens")):
        st = lib.qmha_attend_cached_varlen(cache, *args, CAUSAL, None)
        assert st == 1 and cause in lib.qmha_last_error().decode(), (args, lib.qmha_last_error())
        assert lib.qmha_kv_cache_len(cache) == 0
    assert lib.qmha_attend_cached_varlen(None, DUMMY, DUMMY, 32, DUMMY, CAUSAL, None) == 1


def has_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except ImportError:
        return False


@pytest.mark.skipif(has_gpu(), reason="needs a machine without a GPU: the launch itself must fail")
def test_calls_that_pass_the_checks_reach_the_launch(lib, cache):
    """Unlike qmha_attend_cached, the varlen attend does not look at the host length (0 here), and an unmasked one
    does not need a full cache: both calls get as far as the launch, which fails without a device, and len stays 0."""
    assert lib.qmha_kv_cache_append_at(cache, DUMMY, DUMMY, 64, DUMMY, None) == 2, lib.qmha_last_error()
    assert lib.qmha_attend_cached_varlen(cache, DUMMY, DUMMY, 32, DUMMY, CAUSAL, None) == 2, lib.qmha_last_error()
    assert lib.qmha_attend_cached_varlen(cache, DUMMY, DUMMY, 288, DUMMY, 0, None) == 2, lib.qmha_last_error()  # Nq > cap, no mask
    assert lib.qmha_kv_cache_len(cache) == 0


def test_library_has_the_ten_new_kernels_beside_the_old(lib):
    path = os.path.join(ROOT, "quantizedmha_amd", "lib", "libqmha.so")
    syms = subprocess.run(["nm", path], capture_output=True, text=True, check=True).stdout
    main = sorted(set(re.findall(r"__device_stub__(qmha_fa_(?:int8|f16)_varlen_kernel)ILi(\d+)E", syms)))
    assert main == [("qmha_fa_f16_varlen_kernel", "128"), ("qmha_fa_f16_varlen_kernel", "64"),
                    ("qmha_fa_int8_varlen_kernel", "128"), ("qmha_fa_int8_varlen_kernel", "32"),
                    ("qmha_fa_int8_varlen_kernel", "64")], main
    # the append template over PlacedRow
    place = append_syms.append(syms, row="PlacedRow")
    assert place == [("qmha_kv_append_f16_kernel", "PlacedRow", "128"), ("qmha_kv_append_f16_kernel", "PlacedRow", "64"),
                     ("qmha_kv_append_int8_kernel", "PlacedRow", "128"), ("qmha_kv_append_int8_kernel", "PlacedRow", "32"),
                     ("qmha_kv_append_int8_kernel", "PlacedRow", "64")], place
    # one instance of each: no second geometry, no dumping twin
    assert len(set(re.findall(r"__device_stub__(qmha_fa_\w+?_varlen_kernel\w*)", syms))) == 5
    append_syms.check_family(syms)
    # what the library held before: fifteen masked main kernels, five append kernels
    masked = set(re.findall(r"__device_stub__(qmha_fa_\w+?_masked_kernel)ILi(\d+)ENS_\d+([A-Za-z]+?)E(\w*)", syms))
    assert len(masked) == 15 and {m[2] for m in masked} == {"SquareCausal", "Rect", "Grouped"}, sorted(masked)
    append = append_syms.append(syms, row="HostRow")
    assert append == append_syms.want_append(("HostRow",)) and len(append) == 5, append


@pytest.mark.parametrize("cls", ["KVCache", "GroupedKVCache"])
def test_python_binding_has_the_two_methods(cls):
    from quantizedmha_amd import torch_ext
    c = getattr(torch_ext, cls)
    assert list(inspect.signature(c.append_at).parameters) == ["self", "K", "V", "pos"]
    sig = inspect.signature(c.attend_varlen)
    assert list(sig.parameters) == ["self", "Q", "lens", "causal", "out"]
    assert sig.parameters["causal"].default is True and sig.parameters["out"].default is None


@pytest.mark.parametrize("cls", ["KVCache", "GroupedKVCache"])
def test_compiled_module_has_the_two_methods(lib, cls):
    import sys
    from quantizedmha_amd import _lib
    sys.path.insert(0, _lib.LIB_DIR)
    try:
        import torch_ext
    finally:
        sys.path.pop(0)
    c = getattr(torch_ext, cls)
    doc = c.append_at.__doc__
    assert re.search(r"append_at\(self: [\w.]*KVCache, K: torch\.Tensor, V: torch\.Tensor, pos: torch\.Tensor\) -> None", doc), doc
    doc = c.attend_varlen.__doc__
    assert re.search(r"attend_varlen\(self: [\w.]*KVCache, Q: torch\.Tensor, lens: torch\.Tensor, causal: bool = True, "
                     r"out: (Optional\[torch\.Tensor\]|torch\.Tensor \| None) = None\) -> torch\.Tensor", doc), doc
