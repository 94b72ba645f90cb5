"""CPU tests of grouped-query attention: qmha_solve_gqa and qmha_kv_cache_create_gqa.

Every check of the two entry points runs before any HIP call, so each rejection is reached here with dummy pointers
(as tests/test_rect_cpu.py and tests/test_kvcache_cpu.py do).  There is no size function of its own: the scratch and
the cache are those of a call with h_kv heads.  The shipped library holds exactly five grouped main kernels (the Grouped
instances of the masked templates), no dumping twin of them, and still ten masked ones of the other two geometries.
"""
import ctypes
import os
import re
import subprocess

import pytest

from tests import gpu_support as gs
from tests.gpu_support import CAUSAL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FA, V1A, INT8, UNFUSED, FA_MFMA, INT8_PT = 0, 1, 2, 3, 4, 5  # the C-ABI's variant ids, not gpu_support's names
MEM = 0x10000  # 256-byte aligned, never dereferenced: checks run first
DUMMY = ctypes.c_void_p(0x1000)
BUILT = [({gs.INT8: INT8, gs.F16: V1A}[v], d) for v, d in gs.BUILT]


@pytest.fixture(scope="module")
def lib():
    from tools.build import build
    build(verbose=False)
    from quantizedmha_amd import _lib
    return _lib.load()


def solve_gqa(lib, B=2, Nq=64, Nk=128, d_model=256, h=4, h_kv=2, vid=INT8, flags=0, ws=None, ws_bytes=0, Q=DUMMY, O=DUMMY):
    st = lib.qmha_solve_gqa(Q, DUMMY, DUMMY, O, B, Nq, Nk, d_model, h, h_kv, vid, flags, ws, ws_bytes, None)
    return st, lib.qmha_last_error().decode()


def create_gqa(lib, B=2, cap=256, d_model=256, h=4, h_kv=2, vid=INT8, mem=MEM, nbytes=None):
    """(status, message, handle); nbytes defaults to the stated size: qmha_workspace_size at h_kv heads."""
    if nbytes is None:
        nbytes = lib.qmha_workspace_size(B, cap, h_kv * (d_model // h), h_kv, vid) if h_kv > 0 else 1 << 30
    handle = ctypes.c_void_p()
    st = lib.qmha_kv_cache_create_gqa(ctypes.byref(handle), ctypes.c_void_p(mem) if mem else None, nbytes, B, cap, d_model,
                                      h, h_kv, vid)
    return st, lib.qmha_last_error().decode(), handle


def test_symbols_are_exported_and_declared(lib):
    from quantizedmha_amd import _lib
    header = open(os.path.join(ROOT, "include", "launchers.h")).read()
    for name in ("qmha_solve_gqa", "qmha_kv_cache_create_gqa"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
    # the header states the size rule: there is no qmha_*gqa*_size / _bytes function
    assert "qmha_workspace_size(B, Nk, h_kv * (d_model / h), h_kv, variant)" in header
    assert not re.search(r"qmha_\w*gqa\w*(size|bytes)\s*\(", header)


@pytest.mark.parametrize("h,h_kv", [(4, 0), (4, -1), (4, 5), (4, 8), (4, 3), (6, 4)])
def test_bad_kv_head_counts_are_invalid(lib, h, h_kv):
    st, msg = solve_gqa(lib, d_model=64 * h, h=h, h_kv=h_kv)
    assert st == 1 and "h_kv" in msg, (st, msg)
    st, msg, handle = create_gqa(lib, d_model=64 * h, h=h, h_kv=h_kv, nbytes=1 << 30)
    assert st == 1 and "h_kv" in msg and not handle.value, (st, msg)


@pytest.mark.parametrize("h_kv", [2, 4])  # grouped, and h_kv == h (the checks of qmha_solve_rect)
@pytest.mark.parametrize("kw,cause", [
    (dict(Nq=40), "Nq must be a multiple of 32"),
    (dict(Nk=100), "Nk must be a multiple of 32"),
    (dict(Nq=0), "positive"),
    (dict(Nq=160, Nk=96, flags=CAUSAL), "Nk >= Nq"),
    (dict(flags=2), "flag"), (dict(flags=0x80000001), "flag"),
    (dict(d_model=250), "divisible"),
    (dict(vid=7), "unknown variant"),
    (dict(Q=None), "null"), (dict(O=None), "null"),
])
def test_solve_rejections(lib, h_kv, kw, cause):
    st, msg = solve_gqa(lib, h_kv=h_kv, **kw)
    assert st == 1 and cause in msg, (st, msg)


@pytest.mark.parametrize("vid,d", BUILT)
@pytest.mark.parametrize("Nq,Nk", [(64, 128), (128, 128)])  # square calls take the grouped path too
def test_workspace_one_byte_short_is_refused(lib, vid, d, Nq, Nk):
    B, h, h_kv = 2, 4, 2
    need = lib.qmha_workspace_size(B, Nk, h_kv * d, h_kv, vid)
    assert need > 0
    st, msg = solve_gqa(lib, B=B, Nq=Nq, Nk=Nk, d_model=h * d, h=h, h_kv=h_kv, vid=vid, ws=ctypes.c_void_p(MEM), ws_bytes=need - 1)
    assert st == 1 and "workspace too small" in msg, (st, msg)
    st, msg, handle = create_gqa(lib, B=B, cap=Nk, d_model=h * d, h=h, h_kv=h_kv, vid=vid, nbytes=need - 1)
    assert st == 1 and "too small" in msg and not handle.value, (st, msg)
    st, msg, handle = create_gqa(lib, B=B, cap=Nk, d_model=h * d, h=h, h_kv=h_kv, vid=vid, nbytes=need)
    assert st == 0 and handle.value, (st, msg)
    lib.qmha_kv_cache_destroy(handle)


@pytest.mark.parametrize("vid,name,d_model,h", [
    (FA, "fa", 256, 4), (UNFUSED, "unfused", 256, 4), (FA_MFMA, "fa_mfma", 256, 4), (INT8_PT, "fa_tc_int8_pt", 256, 4),
    (V1A, "fa_tc_v1a", 128, 4),  # fp16 d = 32: int8 only
])
@pytest.mark.parametrize("Nq,Nk,flags", [(64, 128, 0), (64, 128, CAUSAL), (128, 128, 0)])
def test_unsupported_grouped_combinations_are_nosys(lib, vid, name, d_model, h, Nq, Nk, flags):
    st, msg = solve_gqa(lib, Nq=Nq, Nk=Nk, d_model=d_model, h=h, h_kv=2, vid=vid, flags=flags)
    assert st == 4 and name in msg and f"d = {d_model // h}" in msg and "grouped-query" in msg, (st, msg)
    st, msg, handle = create_gqa(lib, cap=Nk, d_model=d_model, h=h, h_kv=2, vid=vid, nbytes=1 << 30)
    assert st == 4 and not handle.value and name in msg and f"d = {d_model // h}" in msg and "grouped-query" in msg, (st, msg)


@pytest.mark.parametrize("vid,d", BUILT)
def test_size_identity(lib, vid, d):
    """The grouped scratch and cache are those of h_kv heads: exactly 1 / G of the multi-head cache when every
    array of the grouped carve is a multiple of 256 bytes (B h_kv cap / 32 scales a multiple of 64), as here."""
    for B, cap, h, h_kv in ((2, 1024, 4, 2), (16, 4096, 16, 4), (4, 512, 8, 1)):
        G = h // h_kv
        grouped = lib.qmha_workspace_size(B, cap, h_kv * d, h_kv, vid)
        assert grouped == lib.qmha_kv_cache_bytes(B, cap, h_kv * d, h_kv, vid) > 0
        assert grouped * G == lib.qmha_kv_cache_bytes(B, cap, h * d, h, vid), (B, cap, h, h_kv)


@pytest.fixture
def cache(lib):
    st, msg, handle = create_gqa(lib, B=2, cap=256, d_model=256, h=4, h_kv=2)
    assert st == 0 and handle.value, (st, msg)
    yield handle
    lib.qmha_kv_cache_destroy(handle)


def test_grouped_cache_rejections_leave_the_length(lib, cache):
    assert lib.qmha_kv_cache_len(cache) == 0
    for n, cause in ((48, "multiple of 32"), (0, "multiple of 32"), (288, "exceed cap")):
        st = lib.qmha_kv_cache_append(cache, DUMMY, DUMMY, n, None)
        assert st == 1 and cause in lib.qmha_last_error().decode(), (n, st, lib.qmha_last_error())
        assert lib.qmha_kv_cache_len(cache) == 0
    for Nq, flags, cause in ((32, CAUSAL, "len >= Nq"), (32, 0, "no unmasked mode"), (32, 2, "flag"),
                             (40, CAUSAL, "Nq must be a multiple of 32")):
        st = lib.qmha_attend_cached(cache, DUMMY, DUMMY, Nq, flags, None)
        assert st == 1 and cause in lib.qmha_last_error().decode(), (Nq, flags, st, lib.qmha_last_error())
    assert lib.qmha_kv_cache_truncate(cache, 32) == 1
    assert lib.qmha_kv_cache_len(cache) == 0


@pytest.mark.parametrize("kw,cause", [
    (dict(cap=100), "cap must be a multiple of 32"),
    (dict(mem=MEM + 16), "256-byte aligned"),
    (dict(mem=0), "null"),
    (dict(vid=7), "unknown variant"),
])
def test_create_invalid_arguments(lib, kw, cause):
    st, msg, handle = create_gqa(lib, nbytes=1 << 30, **kw)
    assert st == 1 and cause in msg and not handle.value, (st, msg)


def test_equal_head_counts_are_the_multi_head_entry_points(lib):
    """h_kv == h: the checks, sizes and messages of qmha_solve_rect / qmha_kv_cache_create (what is enqueued is
    compared on the GPU)."""
    st, msg = solve_gqa(lib, Nq=64, Nk=128, d_model=256, h=4, h_kv=4, vid=FA)
    assert st == 4 and "rectangular attention" in msg and "grouped-query" not in msg, (st, msg)
    need = lib.qmha_workspace_size(2, 128, 256, 4, INT8)
    st, msg = solve_gqa(lib, h_kv=4, ws=ctypes.c_void_p(MEM), ws_bytes=need - 1)
    assert st == 1 and "workspace too small" in msg, (st, msg)
    st, msg, handle = create_gqa(lib, h_kv=4, vid=FA, nbytes=1 << 30)
    assert st == 4 and "cache" in msg and "grouped-query" not in msg and not handle.value, (st, msg)
    st, msg, handle = create_gqa(lib, h_kv=4, nbytes=lib.qmha_kv_cache_bytes(2, 256, 256, 4, INT8) - 1)
    assert st == 1 and "too small" in msg and not handle.value, (st, msg)


def test_library_has_five_grouped_kernels_and_ten_masked(lib):
    """The grouped kernels are the Grouped instances of the masked templates: five of them, beside the ten of the
    SquareCausal and Rect geometries."""
    path = os.path.join(ROOT, "quantizedmha_amd", "lib", "libqmha.so")
    syms = subprocess.run(["nm", path], capture_output=True, text=True, check=True).stdout
    masked = set(re.findall(r"__device_stub__(qmha_fa_\w+?_masked_kernel)ILi(\d+)ENS_\d+([A-Za-z]+?)E(\w*)", syms))
    stubs = sorted((n, d, rest) for n, d, g, rest in masked if g == "Grouped")
    assert [(n, d) for n, d, _ in stubs] == [("qmha_fa_f16_masked_kernel", "128"), ("qmha_fa_f16_masked_kernel", "64"),
                                             ("qmha_fa_int8_masked_kernel", "128"), ("qmha_fa_int8_masked_kernel", "32"),
                                             ("qmha_fa_int8_masked_kernel", "64")], stubs
    # no template argument beyond (D, geometry): no dumping twin, no second instance
    assert all(rest.startswith("EEv") and "Dumping" not in rest for _, _, rest in stubs), stubs
    assert "_gqa_kernel" not in syms
    assert not re.search(r"Dumping\w*Grouped", syms)
    assert len(masked) == 15, sorted(masked)


def test_python_binding_accepts_num_kv_heads():
    import inspect
    from quantizedmha_amd import torch_ext
    sig = inspect.signature(torch_ext.flash_solve_gqa)
    assert list(sig.parameters) == ["Q", "K", "V", "d_model", "num_heads", "num_kv_heads", "kernel", "out", "causal"]
    assert sig.parameters["num_kv_heads"].default is None and sig.parameters["causal"].default is False
    sig = inspect.signature(torch_ext.GroupedKVCache.__init__)
    assert list(sig.parameters) == ["self", "B", "cap", "d_model", "num_heads", "num_kv_heads", "kernel", "device"]
    assert sig.parameters["num_kv_heads"].default is None and sig.parameters["kernel"].default == "fa_tc_int8_b"
    assert issubclass(torch_ext.GroupedKVCache, torch_ext.KVCache)
    torch = pytest.importorskip("torch")
    with pytest.raises(RuntimeError, match="Inputs must be CUDA tensors"):
        torch_ext.flash_solve_gqa(torch.zeros(64, 128), torch.zeros(128, 64), torch.zeros(128, 64), 128, 4, 2)


def test_compiled_module_accepts_num_kv_heads(lib):
    import sys
    from quantizedmha_amd import _lib
    sys.path.insert(0, _lib.LIB_DIR)
    try:
        import torch_ext
    finally:
        sys.path.pop(0)
    assert "num_kv_heads" in torch_ext.flash_solve_gqa.__doc__
    assert "num_kv_heads" in torch_ext.GroupedKVCache.__init__.__doc__
    assert issubclass(torch_ext.GroupedKVCache, torch_ext.KVCache)
