"""CPU tests of the paged K/V cache: qmha_kv_cache_paged_bytes, qmha_kv_cache_create_paged,
qmha_kv_cache_append_paged and qmha_attend_cached_paged.

Every host check of the calls runs before any HIP call, so they are reached here with dummy pointers (as
tests/test_tokens_cpu.py does).  The shipped library holds five paged main kernels and five paged append kernels under
names of their own, beside the kernels it held before.  And the row map the kernels implement -- row -> page, row in
page, group index in the pool -- is restated in numpy and held to a brute-force gather.
"""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from tests import append_syms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAUSAL = 1
V1A, INT8 = 1, 2
MEM = 0x10000  # 256-byte aligned, never dereferenced: checks run first
DUMMY = ctypes.c_void_p(0x1000)
B, NUM_PAGES, PAGE_ROWS, MAX_PAGES = 2, 8, 64, 4  # cap = 256
CAP = MAX_PAGES * PAGE_ROWS
# (d_model, h, h_kv) at d = 64
KINDS = {"multi-head": (128, 2, 2), "grouped": (256, 4, 2)}


@pytest.fixture(scope="module")
def lib():
    from tools.build import build
    build(verbose=False)
    from quantizedmha_amd import _lib
    return _lib.load()


def make_paged(lib, kind, variant=INT8):
    d_model, h, h_kv = KINDS[kind]
    handle = ctypes.c_void_p()
    nbytes = lib.qmha_kv_cache_paged_bytes(NUM_PAGES, PAGE_ROWS, d_model, h, h_kv, variant)
    st = lib.qmha_kv_cache_create_paged(ctypes.byref(handle), ctypes.c_void_p(MEM), nbytes, B, NUM_PAGES, PAGE_ROWS, MAX_PAGES,
                                        d_model, h, h_kv, variant)
    assert st == 0 and handle.value, (st, lib.qmha_last_error())
    return handle


def make_contiguous(lib, kind, variant=INT8):
    d_model, h, h_kv = KINDS[kind]
    handle = ctypes.c_void_p()
    nbytes = lib.qmha_kv_cache_bytes(B, CAP, h_kv * 64, h_kv, variant)
    st = lib.qmha_kv_cache_create_gqa(ctypes.byref(handle), ctypes.c_void_p(MEM), nbytes, B, CAP, d_model, h, h_kv, variant)
    assert st == 0 and handle.value, (st, lib.qmha_last_error())
    return handle


@pytest.fixture(params=list(KINDS))
def cache(lib, request):
    handle = make_paged(lib, request.param)
    yield handle
    lib.qmha_kv_cache_destroy(handle)


TAIL = 2 * B * 32 * 2 * 64 * 4  # K and V, B sequence slots, 32 rows of h_kv d = 128 fp32


def err(lib):
    return lib.qmha_last_error().decode()


# ---- the declarations and the exports (these fail on a library without the feature) -------------------------------------
def test_header_declares_the_four_calls():
    header = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "launchers.h")).read())
    for decl in ("size_t qmha_kv_cache_paged_bytes(int num_pages, int page_rows, int d_model, int h, int h_kv, int variant);",
                 "int qmha_kv_cache_create_paged(qmha_kv_cache_t **out, void *mem, size_t bytes, int B, int num_pages, int page_rows, "
                 "int max_pages, int d_model, int h, int h_kv, int variant);",
                 "int qmha_kv_cache_append_paged(qmha_kv_cache_t *c, const float *K, const float *V, int n, const int32_t *pos, "
                 "const int32_t *table, void *stream);",
                 "int qmha_attend_cached_paged(qmha_kv_cache_t *c, const float *Q, float *O, int Nq, const int32_t *lens, "
                 "const int32_t *table, unsigned flags, void *stream);"):
        assert decl in header, decl
    # the header states the sharing rule
    assert "prefix sharing" in header and "caller's error" in header


def test_library_exports_the_four_calls(lib):
    from quantizedmha_amd import _lib
    vp, i, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
    for name, res, argtypes in (("qmha_kv_cache_paged_bytes", sz, [i] * 6),
                                ("qmha_kv_cache_create_paged", i, [ctypes.POINTER(vp), vp, sz] + [i] * 8),
                                ("qmha_kv_cache_append_paged", i, [vp, vp, vp, i, vp, vp, vp]),
                                ("qmha_attend_cached_paged", i, [vp, vp, vp, i, vp, vp, ctypes.c_uint, vp])):
        fn = getattr(lib, name)  # AttributeError on a library without the symbol
        assert fn.restype is res and list(fn.argtypes) == argtypes, name
    path = os.path.join(_lib.LIB_DIR, "libqmha.so")
    dyn = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    for name in ("qmha_kv_cache_paged_bytes", "qmha_kv_cache_create_paged", "qmha_kv_cache_append_paged", "qmha_attend_cached_paged"):
        assert re.search(rf" T {name}$", dyn, re.M), name


# ---- the pool is the existing carve ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [INT8, V1A])
@pytest.mark.parametrize("kind", list(KINDS))
def test_paged_bytes_is_the_workspace_of_the_pool(lib, kind, variant):
    d_model, h, h_kv = KINDS[kind]
    d = d_model // h
    for num_pages, page_rows in ((1, 64), (8, 64), (16, 128), (5, 192), (1024, 256)):
        got = lib.qmha_kv_cache_paged_bytes(num_pages, page_rows, d_model, h, h_kv, variant)
        assert got > 0 and got == lib.qmha_workspace_size(num_pages, page_rows, h_kv * d, h_kv, variant), (num_pages, page_rows)
    # pages of a contiguous cache's rows cost what the cache costs (up to the 256-byte rounding of each array)
    assert lib.qmha_kv_cache_paged_bytes(B * MAX_PAGES, PAGE_ROWS, d_model, h, h_kv, variant) == \
        lib.qmha_kv_cache_bytes(B, CAP, h_kv * d, h_kv, variant)
    assert lib.qmha_kv_cache_paged_bytes(0, 64, d_model, h, h_kv, variant) == 0
    assert lib.qmha_kv_cache_paged_bytes(8, 64, d_model, h, 0, variant) == 0


# ---- create ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(KINDS))
def test_create_paged_rejections(lib, kind):
    d_model, h, h_kv = KINDS[kind]
    nbytes = lib.qmha_kv_cache_paged_bytes(NUM_PAGES, PAGE_ROWS, d_model, h, h_kv, INT8)
    handle = ctypes.c_void_p()

    def create(mem=MEM, nb=nbytes, b=B, num_pages=NUM_PAGES, page_rows=PAGE_ROWS, max_pages=MAX_PAGES, dm=d_model, hh=h, hk=h_kv,
               variant=INT8, out=True):
        handle.value = 0x55
        st = lib.qmha_kv_cache_create_paged(ctypes.byref(handle) if out else None, ctypes.c_void_p(mem) if mem else None, nb, b,
                                            num_pages, page_rows, max_pages, dm, hh, hk, variant)
        assert st == 0 or not handle.value or not out  # a refused create leaves a null handle
        return st

    for page_rows in (0, 32, 96, 100, -64):
        assert create(page_rows=page_rows) == 1 and "page_rows" in err(lib) and "multiple of 64" in err(lib), page_rows
    for num_pages in (0, -1):
        assert create(num_pages=num_pages) == 1 and "num_pages" in err(lib), num_pages
    for max_pages in (0, -3):
        assert create(max_pages=max_pages) == 1 and "max_pages" in err(lib), max_pages
    assert create(mem=None) == 1 and "null cache memory" in err(lib)
    assert create(out=False) == 1 and "null cache handle" in err(lib)
    assert create(mem=MEM + 64) == 1 and "256-byte aligned" in err(lib)
    assert create(nb=nbytes - 1) == 1 and "too small" in err(lib) and "qmha_kv_cache_paged_bytes" in err(lib)
    assert create(b=0) == 1 and "must be positive" in err(lib)
    assert create(hk=3) == 1 and "h_kv must divide h" in err(lib)
    assert create(hk=0) == 1 and "h_kv must divide h" in err(lib)
    assert create(dm=d_model + 1) == 1 and "divisible by h" in err(lib)
    # "not built", as qmha_kv_cache_create_gqa: fp16 has no d = 32, the fp32 variant no cache at all
    assert create(dm=32 * h, variant=V1A) == 4 and "not built" in err(lib)
    assert create(variant=0) == 4 and "not built" in err(lib)
    assert create() == 0, err(lib)
    lib.qmha_kv_cache_destroy(handle)


# ---- the calls' host rejections ------------------------------------------------------------------------------------------
def test_append_paged_rejections(lib, cache):
    assert lib.qmha_kv_cache_attach_tail(cache, ctypes.c_void_p(MEM), TAIL) == 0
    for n in (0, -1, CAP + 1, CAP + 32):
        st = lib.qmha_kv_cache_append_paged(cache, DUMMY, DUMMY, n, DUMMY, DUMMY, None)
        assert st == 1 and "1 <= n <= cap" in err(lib), (n, st, err(lib))
    for args, cause in (((None, DUMMY, 1, DUMMY, DUMMY), "null tensor"), ((DUMMY, None, 1, DUMMY, DUMMY), "null tensor"),
                        ((DUMMY, DUMMY, 1, None, DUMMY), "null pos"), ((DUMMY, DUMMY, 1, DUMMY, None), "null table")):
        assert lib.qmha_kv_cache_append_paged(cache, *args, None) == 1 and cause in err(lib), (args, err(lib))
    assert lib.qmha_kv_cache_append_paged(None, DUMMY, DUMMY, 1, DUMMY, DUMMY, None) == 1 and "null cache" in err(lib)
    assert lib.qmha_kv_cache_len(cache) == 0


def test_append_paged_needs_the_tail_on_an_int8_cache(lib, cache):
    for n in (1, 64, CAP):
        st = lib.qmha_kv_cache_append_paged(cache, DUMMY, DUMMY, n, DUMMY, DUMMY, None)
        assert st == 1 and "needs its tail" in err(lib), (n, st, err(lib))


def test_attend_paged_rejections(lib, cache):
    for Nq, flags, cause in ((1, 0, "must be QMHA_FLAG_CAUSAL"), (32, 2, "must be QMHA_FLAG_CAUSAL"), (5, 3, "must be QMHA_FLAG_CAUSAL"),
                             (1, 0x80000001, "must be QMHA_FLAG_CAUSAL"), (0, CAUSAL, "1 <= Nq <= cap"),
                             (-5, CAUSAL, "1 <= Nq <= cap"), (CAP + 1, CAUSAL, "1 <= Nq <= cap")):
        st = lib.qmha_attend_cached_paged(cache, DUMMY, DUMMY, Nq, DUMMY, DUMMY, flags, None)
        assert st == 1 and cause in err(lib), (Nq, flags, st, err(lib))
    for args, cause in (((None, DUMMY, 1, DUMMY, DUMMY), "null tensor"), ((DUMMY, None, 1, DUMMY, DUMMY), "null tensor"),
                        ((DUMMY, DUMMY, 1, None, DUMMY), "null lens"), ((DUMMY, DUMMY, 1, DUMMY, None), "null table")):
        st = lib.qmha_attend_cached_paged(cache, *args, CAUSAL, None)
        assert st == 1 and cause in err(lib), (args, err(lib))
    assert lib.qmha_attend_cached_paged(None, DUMMY, DUMMY, 1, DUMMY, DUMMY, CAUSAL, None) == 1 and "null cache" in err(lib)


def test_contiguous_calls_refuse_a_paged_cache(lib, cache):
    assert lib.qmha_kv_cache_attach_tail(cache, ctypes.c_void_p(MEM), TAIL) == 0
    for call in (lambda: lib.qmha_kv_cache_append(cache, DUMMY, DUMMY, 32, None),
                 lambda: lib.qmha_attend_cached(cache, DUMMY, DUMMY, 32, CAUSAL, None),
                 lambda: lib.qmha_kv_cache_append_at(cache, DUMMY, DUMMY, 32, DUMMY, None),
                 lambda: lib.qmha_attend_cached_varlen(cache, DUMMY, DUMMY, 32, DUMMY, CAUSAL, None),
                 lambda: lib.qmha_kv_cache_append_tokens(cache, DUMMY, DUMMY, 1, DUMMY, None),
                 lambda: lib.qmha_attend_cached_tokens(cache, DUMMY, DUMMY, 1, DUMMY, CAUSAL, None),
                 lambda: lib.qmha_kv_cache_truncate(cache, 0)):
        assert call() == 1 and "the cache is paged" in err(lib), err(lib)
    assert lib.qmha_kv_cache_len(cache) == 0


@pytest.mark.parametrize("kind", list(KINDS))
def test_paged_calls_refuse_a_contiguous_cache(lib, kind):
    c = make_contiguous(lib, kind)
    try:
        assert lib.qmha_kv_cache_attach_tail(c, ctypes.c_void_p(MEM), TAIL) == 0
        assert lib.qmha_kv_cache_append_paged(c, DUMMY, DUMMY, 1, DUMMY, DUMMY, None) == 1 and "the cache is contiguous" in err(lib)
        assert lib.qmha_attend_cached_paged(c, DUMMY, DUMMY, 1, DUMMY, DUMMY, CAUSAL, None) == 1 and "the cache is contiguous" in err(lib)
    finally:
        lib.qmha_kv_cache_destroy(c)


# ---- the tail belongs to the sequence slots --------------------------------------------------------------------------------
def test_tail_size_and_attachment(lib, cache):
    assert lib.qmha_kv_cache_tail_bytes(cache) == TAIL  # [2][B][32][h_kv d]: B slots, whatever num_pages is
    for mem, nbytes, cause in ((MEM, TAIL - 1, "too small"), (None, TAIL, "null tail"), (MEM + 64, TAIL, "256-byte aligned")):
        st = lib.qmha_kv_cache_attach_tail(cache, ctypes.c_void_p(mem) if mem else None, nbytes)
        assert st == 1 and cause in err(lib), (mem, nbytes, st, err(lib))
    st = lib.qmha_kv_cache_append_paged(cache, DUMMY, DUMMY, 1, DUMMY, DUMMY, None)  # a refused tail was not attached
    assert st == 1 and "needs its tail" in err(lib)
    assert lib.qmha_kv_cache_attach_tail(cache, ctypes.c_void_p(MEM), TAIL) == 0, err(lib)


@pytest.mark.parametrize("kind", list(KINDS))
def test_an_fp16_paged_cache_needs_no_tail(lib, kind):
    c = make_paged(lib, kind, V1A)
    try:
        assert lib.qmha_kv_cache_tail_bytes(c) == 0
        assert lib.qmha_kv_cache_attach_tail(c, None, 0) == 0, err(lib)
    finally:
        lib.qmha_kv_cache_destroy(c)


def has_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except ImportError:
        return False


@pytest.mark.skipif(has_gpu(), reason="needs a machine without a GPU: the launch itself must fail")
def test_calls_that_pass_the_checks_reach_the_launch(lib, cache):
    assert lib.qmha_kv_cache_attach_tail(cache, ctypes.c_void_p(MEM), TAIL) == 0
    for n in (1, 33, CAP):
        assert lib.qmha_kv_cache_append_paged(cache, DUMMY, DUMMY, n, DUMMY, DUMMY, None) == 2, err(lib)
    for Nq in (1, 5, 40, CAP):
        assert lib.qmha_attend_cached_paged(cache, DUMMY, DUMMY, Nq, DUMMY, DUMMY, CAUSAL, None) == 2, err(lib)


# ---- the kernels ---------------------------------------------------------------------------------------------------------
def test_library_has_the_ten_paged_kernels_beside_the_old(lib):
    path = os.path.join(ROOT, "quantizedmha_amd", "lib", "libqmha.so")
    syms = subprocess.run(["nm", path], capture_output=True, text=True, check=True).stdout
    # the cache kernel template over Paged
    main = sorted(set(re.findall(r"__device_stub__(qmha_fa_(?:int8|f16)_cache_kernel)ILi(\d+)ENS_5PagedEEEv", syms)))
    assert main == [("qmha_fa_f16_cache_kernel", "128"), ("qmha_fa_f16_cache_kernel", "64"),
                    ("qmha_fa_int8_cache_kernel", "128"), ("qmha_fa_int8_cache_kernel", "32"),
                    ("qmha_fa_int8_cache_kernel", "64")], main
    # the rows template over UniformRows and PagedTable
    append = append_syms.rows(syms, src="UniformRows", dst="PagedTable")
    u, t = "UniformRows", "PagedTable"
    assert append == [("qmha_kv_rows_f16_kernel", u, t, "128"), ("qmha_kv_rows_f16_kernel", u, t, "64"),
                      ("qmha_kv_rows_int8_kernel", u, t, "128"), ("qmha_kv_rows_int8_kernel", u, t, "32"),
                      ("qmha_kv_rows_int8_kernel", u, t, "64")], append
    # one instance of each: no second geometry, no dumping twin
    assert len(set(re.findall(r"__device_stub__(qmha_fa_\w+?_cache_kernelILi\d+ENS_5Paged\w*)", syms))) == 5
    assert len(set(re.findall(r"__device_stub__(qmha_fa_\w+?_cache_kernel\w*)", syms))) == 20  # four geometries, nothing else
    append_syms.check_family(syms)
    # what the library held before
    masked = set(re.findall(r"__device_stub__(qmha_fa_\w+?_masked_kernel)ILi(\d+)ENS_\d+([A-Za-z]+?)E(\w*)", syms))
    assert len(masked) == 15 and {m[2] for m in masked} == {"SquareCausal", "Rect", "Grouped"}, sorted(masked)
    assert len(set(re.findall(r"__device_stub__(qmha_fa_\w+?_varlen_kernel\w*)", syms))) == 5
    assert len(set(re.findall(r"__device_stub__(qmha_fa_\w+?_cache_kernelILi\d+ENS_6Ragged\w*)", syms))) == 5
    assert append_syms.rows(syms, src="UniformRows", dst="ContiguousRows") == append_syms.want_rows(("UniformRows",), ("ContiguousRows",))
    assert append_syms.append(syms, row="HostRow") == append_syms.want_append(("HostRow",))
    assert append_syms.append(syms, row="PlacedRow") == append_syms.want_append(("PlacedRow",))


# ---- the bindings ----------------------------------------------------------------------------------------------------------
def test_python_binding_has_the_class():
    from quantizedmha_amd import torch_ext
    c = torch_ext.PagedKVCache
    sig = inspect.signature(c.__init__)
    assert list(sig.parameters) == ["self", "B", "num_pages", "page_rows", "max_pages", "d_model", "num_heads", "num_kv_heads",
                                    "kernel", "device"]
    assert sig.parameters["num_kv_heads"].default is None and sig.parameters["device"].default == "cuda"
    assert list(inspect.signature(c.enable_tokens).parameters) == ["self"]
    assert list(inspect.signature(c.append_paged).parameters) == ["self", "K", "V", "pos", "table"]
    sig = inspect.signature(c.attend_paged)
    assert list(sig.parameters) == ["self", "Q", "lens", "table", "out"] and sig.parameters["out"].default is None


def test_compiled_module_has_the_class(lib):
    import sys
    from quantizedmha_amd import _lib
    sys.path.insert(0, _lib.LIB_DIR)
    try:
        import torch_ext
    finally:
        sys.path.pop(0)
    c = torch_ext.PagedKVCache
    i = r"(int|typing\.SupportsInt)"  # how the pybind11 at hand spells an int64_t argument
    assert re.search(rf"__init__\(self: [\w.]*PagedKVCache, B: {i}, num_pages: {i}, page_rows: {i}, max_pages: {i}, d_model: {i}, "
                     rf"num_heads: {i}, num_kv_heads: (Optional\[{i}\]|{i} \| None) = None, kernel: str = 'fa_tc_int8_b', "
                     r"device: str = 'cuda'\) -> None", c.__init__.__doc__), c.__init__.__doc__
    assert re.search(r"enable_tokens\(self: [\w.]*PagedKVCache\) -> None", c.enable_tokens.__doc__), c.enable_tokens.__doc__
    doc = c.append_paged.__doc__
    assert re.search(r"append_paged\(self: [\w.]*PagedKVCache, K: torch\.Tensor, V: torch\.Tensor, pos: torch\.Tensor, "
                     r"table: torch\.Tensor\) -> None", doc), doc
    doc = c.attend_paged.__doc__
    assert re.search(r"attend_paged\(self: [\w.]*PagedKVCache, Q: torch\.Tensor, lens: torch\.Tensor, table: torch\.Tensor, "
                     r"out: (Optional\[torch\.Tensor\]|torch\.Tensor \| None) = None\) -> torch\.Tensor", doc), doc
    for prop in ("mem", "tail", "cap"):
        assert hasattr(c, prop), prop


# ---- the row map ---------------------------------------------------------------------------------------------------------
def row_map(table, page_rows, h_kv, b, kvh, r):
    """What the kernels compute for row r of sequence b, K/V head kvh: (page, row in page, slice in the pool, index of the
    row's 32-row group in the pool's [num_pages h_kv][page_rows / 32] arrays)."""
    pg = page_rows // 32
    g = r // 32
    page = int(table[b, g // pg])
    sl = page * h_kv + kvh
    return page, r % page_rows, sl, sl * pg + g % pg


@pytest.mark.parametrize("max_pages", [1, 2, 4])
@pytest.mark.parametrize("page_rows", [64, 128, 192])
def test_row_map_against_a_brute_force_gather(page_rows, max_pages):
    """A pool filled with each row's own (sequence, head, row) label through the map; gathering the pool back row by row --
    page table[b][r // page_rows], row r % page_rows -- gives the contiguous labels, for a contiguous and a permuted table."""
    nb, h_kv = 3, 2
    num_pages = nb * max_pages + 3
    cap = max_pages * page_rows
    rng = np.random.default_rng(page_rows + max_pages)
    label = np.arange(nb * h_kv * cap).reshape(nb, h_kv, cap)  # the contiguous cache: [B][h_kv][cap]
    contiguous = np.arange(nb * max_pages, dtype=np.int32).reshape(nb, max_pages)
    permuted = rng.permutation(num_pages)[:nb * max_pages].astype(np.int32).reshape(nb, max_pages)
    gathered = []
    for table in (contiguous, permuted):
        pool = np.full((num_pages * h_kv, page_rows), -1)  # [num_pages h_kv][page_rows]: the carve at B := num_pages, N := page_rows
        groups = np.full((num_pages * h_kv * (page_rows // 32),), -1)
        for b in range(nb):
            for kvh in range(h_kv):
                for r in range(cap):
                    page, rin, sl, gi = row_map(table, page_rows, h_kv, b, kvh, r)
                    assert 0 <= page < num_pages and pool[sl, rin] == -1  # no two rows in one place
                    pool[sl, rin] = label[b, kvh, r]
                    # the group index is the group of that row within the slice: groups do not straddle pages
                    assert gi == sl * (page_rows // 32) + rin // 32
                    assert groups[gi] in (-1, label[b, kvh, r - r % 32])
                    groups[gi] = label[b, kvh, r - r % 32]
        # the brute-force gather
        back = np.empty_like(label)
        for b in range(nb):
            for kvh in range(h_kv):
                for r in range(cap):
                    back[b, kvh, r] = pool[table[b, r // page_rows] * h_kv + kvh, r % page_rows]
        assert np.array_equal(back, label)
        assert (pool == -1).sum() == (num_pages - nb * max_pages) * h_kv * page_rows  # pages no table names stay untouched
        gathered.append(back)
    assert np.array_equal(gathered[0], gathered[1])
    # a stage of two key tiles lies in one page: stage st -> column st // (page_rows / 64), offset st % (page_rows / 64)
    spp = page_rows // 64
    for st in range(cap // 64):
        rows = np.arange(64 * st, 64 * st + 64)
        assert len({r // page_rows for r in rows}) == 1 and rows[0] // page_rows == st // spp
        assert rows[0] % page_rows == (st % spp) * 64
