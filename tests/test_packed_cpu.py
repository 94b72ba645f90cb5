"""CPU tests of the packed-batch calls: qmha_kv_cache_append_packed, qmha_kv_cache_append_paged_packed,
qmha_attend_cached_packed and qmha_attend_cached_paged_packed.

Every host check of the calls runs before any HIP call, so they are reached here with dummy pointers (as
tests/test_tokens_cpu.py does).  The shipped library holds ten packed main kernels and ten packed append kernels under
names of their own, beside the kernels it held before.  And the index arithmetic of the kernels -- the prologue's
validity rules and geometry, the append's items -- is restated in tests/packed_ref.py, tied to the source by verbatim
line checks, and swept exhaustively: no address leaves a sequence's range, no tile lies beyond ceil32(L), no group
beyond the cache.
"""
import ctypes
import inspect
import os
import re
import subprocess

import pytest

from tests import append_syms
from tests import packed_ref as pk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "quantizedmha_amd", "csrc")
CAUSAL = 1
V1A, INT8 = 1, 2
MEM = 0x10000  # 256-byte aligned, never dereferenced: checks run first
DUMMY = ctypes.c_void_p(0x1000)
B, CAP = 2, 256
NUM_PAGES, PAGE_ROWS, MAX_PAGES = 8, 64, 4  # the paged cache's logical capacity is CAP too
# (d_model, h, h_kv, paged) at d = 64
KINDS = {"multi-head": (128, 2, 2, False), "grouped": (256, 4, 2, False), "paged": (256, 4, 2, True)}
TAIL = 2 * B * 32 * 2 * 64 * 4  # K and V, B sequence slots, 32 rows of h_kv d = 128 fp32
NAMES = ("qmha_kv_cache_append_packed", "qmha_kv_cache_append_paged_packed", "qmha_attend_cached_packed",
         "qmha_attend_cached_paged_packed")


@pytest.fixture(scope="module")
def lib():
    from tools.build import build
    build(verbose=False)
    from quantizedmha_amd import _lib
    return _lib.load()


def make(lib, kind, variant=INT8, paged=None):
    d_model, h, h_kv, pg = KINDS[kind]
    pg = pg if paged is None else paged
    handle = ctypes.c_void_p()
    if pg:
        nbytes = lib.qmha_kv_cache_paged_bytes(NUM_PAGES, PAGE_ROWS, d_model, h, h_kv, variant)
        st = lib.qmha_kv_cache_create_paged(ctypes.byref(handle), ctypes.c_void_p(MEM), nbytes, B, NUM_PAGES, PAGE_ROWS, MAX_PAGES,
                                            d_model, h, h_kv, variant)
    else:
        nbytes = lib.qmha_kv_cache_bytes(B, CAP, h_kv * 64, h_kv, variant)
        st = lib.qmha_kv_cache_create_gqa(ctypes.byref(handle), ctypes.c_void_p(MEM), nbytes, B, CAP, d_model, h, h_kv, variant)
    assert st == 0 and handle.value, (st, lib.qmha_last_error())
    return handle


@pytest.fixture(params=list(KINDS))
def cache(lib, request):
    handle = make(lib, request.param)
    handle.paged = KINDS[request.param][3]
    yield handle
    lib.qmha_kv_cache_destroy(handle)


def err(lib):
    return lib.qmha_last_error().decode()


def append(lib, c, K=DUMMY, V=DUMMY, total=8, max_n=4, cu=DUMMY, pos=DUMMY, table=DUMMY, paged=None):
    """The append entry point of the cache's kind (or of `paged`)."""
    if c is not None and getattr(c, "paged", False) if paged is None else paged:
        return lib.qmha_kv_cache_append_paged_packed(c, K, V, total, max_n, cu, pos, table, None)
    return lib.qmha_kv_cache_append_packed(c, K, V, total, max_n, cu, pos, None)


def attend(lib, c, Q=DUMMY, O=DUMMY, total=8, max_nq=4, cu=DUMMY, lens=DUMMY, table=DUMMY, flags=CAUSAL, paged=None):
    if c is not None and getattr(c, "paged", False) if paged is None else paged:
        return lib.qmha_attend_cached_paged_packed(c, Q, O, total, max_nq, cu, lens, table, flags, None)
    return lib.qmha_attend_cached_packed(c, Q, O, total, max_nq, cu, lens, flags, None)


# ---- the declarations and the exports (these fail on a library without the feature) -------------------------------------
def test_header_declares_the_four_calls():
    header = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "launchers.h")).read())
    for decl in ("int qmha_kv_cache_append_packed(qmha_kv_cache_t *c, const float *K, const float *V, int total, int max_n, "
                 "const int32_t *cu, const int32_t *pos, void *stream);",
                 "int qmha_kv_cache_append_paged_packed(qmha_kv_cache_t *c, const float *K, const float *V, int total, int max_n, "
                 "const int32_t *cu, const int32_t *pos, const int32_t *table, void *stream);",
                 "int qmha_attend_cached_packed(qmha_kv_cache_t *c, const float *Q, float *O, int total, int max_nq, "
                 "const int32_t *cu, const int32_t *lens, unsigned flags, void *stream);",
                 "int qmha_attend_cached_paged_packed(qmha_kv_cache_t *c, const float *Q, float *O, int total, int max_nq, "
                 "const int32_t *cu, const int32_t *lens, const int32_t *table, unsigned flags, void *stream);"):
        assert decl in header, decl
    # the header documents the array conventions
    for words in ("DEVICE int32 [B + 1]", "[cu[b], cu[b + 1])", "never becomes an address", "monotone cu"):
        assert words in header, words


def test_library_exports_the_four_calls(lib):
    from quantizedmha_amd import _lib
    vp, i, u = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint
    for name, argtypes in zip(NAMES, ([vp, vp, vp, i, i, vp, vp, vp], [vp, vp, vp, i, i, vp, vp, vp, vp],
                                      [vp, vp, vp, i, i, vp, vp, u, vp], [vp, vp, vp, i, i, vp, vp, vp, u, vp])):
        fn = getattr(lib, name)  # AttributeError on a library without the symbol
        assert fn.restype is i and list(fn.argtypes) == argtypes, name
    path = os.path.join(_lib.LIB_DIR, "libqmha.so")
    dyn = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    for name in NAMES:
        assert re.search(rf" T {name}$", dyn, re.M), name


# ---- the calls' host rejections ------------------------------------------------------------------------------------------
def test_append_packed_rejections(lib, cache):
    assert lib.qmha_kv_cache_attach_tail(cache, ctypes.c_void_p(MEM), TAIL) == 0
    for total in (0, -3):
        assert append(lib, cache, total=total, max_n=1) == 1 and "needs total >= 1" in err(lib), (total, err(lib))
    for total, max_n in ((8, 0), (8, -1), (8, 9), (CAP + 64, CAP + 1), (CAP + 64, CAP + 64)):
        st = append(lib, cache, total=total, max_n=max_n)
        assert st == 1 and "1 <= max_n <= min(total" in err(lib) and f"max_n = {max_n}" in err(lib), (total, max_n, st, err(lib))
    for kw, cause in (({"K": None}, "null tensor"), ({"V": None}, "null tensor"), ({"cu": None}, "null cu"), ({"pos": None}, "null pos")):
        assert append(lib, cache, **kw) == 1 and cause in err(lib), (kw, err(lib))
    if cache.paged:
        assert append(lib, cache, table=None) == 1 and "null table" in err(lib)
    assert append(lib, None, paged=False) == 1 and "null cache" in err(lib)
    assert append(lib, None, paged=True) == 1 and "null cache" in err(lib)
    assert lib.qmha_kv_cache_len(cache) == 0


def test_append_packed_needs_the_tail_on_an_int8_cache(lib, cache):
    for total, max_n in ((1, 1), (300, 64), (CAP, CAP)):
        st = append(lib, cache, total=total, max_n=max_n)
        assert st == 1 and "needs its tail" in err(lib), (total, max_n, st, err(lib))


def test_attend_packed_rejections(lib, cache):
    for flags in (0, 2, 3, 0x80000001):
        assert attend(lib, cache, flags=flags) == 1 and "must be QMHA_FLAG_CAUSAL" in err(lib), (flags, err(lib))
    for total in (0, -3):
        assert attend(lib, cache, total=total, max_nq=1) == 1 and "needs total >= 1" in err(lib), (total, err(lib))
    for total, max_nq in ((8, 0), (8, -5), (8, 9), (CAP + 64, CAP + 1)):
        st = attend(lib, cache, total=total, max_nq=max_nq)
        assert st == 1 and "1 <= max_nq <= min(total" in err(lib) and f"max_nq = {max_nq}" in err(lib), (total, max_nq, st, err(lib))
    for kw, cause in (({"Q": None}, "null tensor"), ({"O": None}, "null tensor"), ({"cu": None}, "null cu"), ({"lens": None}, "null lens")):
        assert attend(lib, cache, **kw) == 1 and cause in err(lib), (kw, err(lib))
    if cache.paged:
        assert attend(lib, cache, table=None) == 1 and "null table" in err(lib)
    assert attend(lib, None, paged=False) == 1 and "null cache" in err(lib)
    assert attend(lib, None, paged=True) == 1 and "null cache" in err(lib)


def test_each_entry_point_refuses_the_other_kind_of_cache(lib, cache):
    assert lib.qmha_kv_cache_attach_tail(cache, ctypes.c_void_p(MEM), TAIL) == 0
    cause = "the cache is paged" if cache.paged else "the cache is contiguous"
    assert append(lib, cache, paged=not cache.paged) == 1 and cause in err(lib), err(lib)
    assert attend(lib, cache, paged=not cache.paged) == 1 and cause in err(lib), err(lib)


@pytest.mark.parametrize("kind", list(KINDS))
def test_an_fp16_cache_needs_no_tail(lib, kind):
    c = make(lib, kind, V1A)
    c.paged = KINDS[kind][3]
    try:
        assert append(lib, c, max_n=0) == 1 and "max_n" in err(lib)  # the checks before the tail's still hold
        assert "needs its tail" not in err(lib)
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
    for total, bound in ((1, 1), (50, 40), (CAP, CAP), (5000, CAP), (5000, 512 if CAP >= 512 else CAP)):
        assert append(lib, cache, total=total, max_n=bound) == 2, err(lib)
        assert attend(lib, cache, total=total, max_nq=bound) == 2, err(lib)


# ---- the kernels ---------------------------------------------------------------------------------------------------------
def test_library_has_the_twenty_packed_kernels_beside_the_old(lib):
    path = os.path.join(ROOT, "quantizedmha_amd", "lib", "libqmha.so")
    syms = subprocess.run(["nm", path], capture_output=True, text=True, check=True).stdout
    sizes = {"int8": ["128", "32", "64"], "f16": ["128", "64"]}
    # the cache kernel template over Packed<Ragged> and Packed<Paged>
    for family, pattern in (("qmha_fa_{}_cache_kernel", r"__device_stub__(qmha_fa_(?:int8|f16)_cache_kernel)ILi(\d+)ENS_6PackedINS_6RaggedEEEEEv"),
                            ("qmha_fa_{}_cache_kernel", r"__device_stub__(qmha_fa_(?:int8|f16)_cache_kernel)ILi(\d+)ENS_6PackedINS_5PagedEEEEEv")):
        got = sorted(set(re.findall(pattern, syms)))
        want = sorted((family.format(p), d) for p, ds in sizes.items() for d in ds)
        assert got == want, (family, got)
    # the rows template over PackedRows, and ContiguousRows or PagedTable
    for dst in ("ContiguousRows", "PagedTable"):
        got = append_syms.rows(syms, src="PackedRows", dst=dst)
        assert got == sorted((f"qmha_kv_rows_{p}_kernel", "PackedRows", dst, d) for p, ds in sizes.items() for d in ds), (dst, got)
    # one instance of each per head size: no second geometry, no dumping twin
    assert len(set(re.findall(r"__device_stub__(qmha_fa_\w+?_cache_kernelILi\d+ENS_6Packed\w*)", syms))) == 10
    assert len(set(re.findall(r"__device_stub__(qmha_fa_\w+?_cache_kernel\w*)", syms))) == 20  # four geometries, nothing else
    assert len(append_syms.rows(syms, src="PackedRows")) == 10
    append_syms.check_family(syms)
    # what the library held before
    masked = set(re.findall(r"__device_stub__(qmha_fa_\w+?_masked_kernel)ILi(\d+)ENS_\d+([A-Za-z]+?)E(\w*)", syms))
    assert len(masked) == 15 and {m[2] for m in masked} == {"SquareCausal", "Rect", "Grouped"}, sorted(masked)
    for family, n in ((r"qmha_fa_\w+?_varlen_kernel\w*", 5), (r"qmha_fa_\w+?_cache_kernelILi\d+ENS_6Ragged\w*", 5),
                      (r"qmha_fa_\w+?_cache_kernelILi\d+ENS_5Paged\w*", 5), (r"qmha_fa_\w+?_split_kernelILi\d+ENS_6Ragged\w*", 5),
                      (r"qmha_fa_\w+?_split_kernelILi\d+ENS_5Paged\w*", 5), (r"qmha_split_combine_kernel\w*", 1)):
        assert len(set(re.findall(rf"__device_stub__({family})", syms))) == n, family
    for dst in ("ContiguousRows", "PagedTable"):
        assert append_syms.rows(syms, src="UniformRows", dst=dst) == append_syms.want_rows(("UniformRows",), (dst,)), dst
    for row in append_syms.ROWS:
        assert append_syms.append(syms, row=row) == append_syms.want_append((row,)), row


# ---- the bindings ----------------------------------------------------------------------------------------------------------
def test_python_binding_has_the_methods():
    from quantizedmha_amd import torch_ext
    for c in (torch_ext.KVCache, torch_ext.GroupedKVCache):
        assert list(inspect.signature(c.append_packed).parameters) == ["self", "K", "V", "cu", "pos", "max_n"]
        sig = inspect.signature(c.attend_packed)
        assert list(sig.parameters) == ["self", "Q", "cu", "lens", "max_nq", "out"] and sig.parameters["out"].default is None
    c = torch_ext.PagedKVCache
    assert list(inspect.signature(c.append_paged_packed).parameters) == ["self", "K", "V", "cu", "pos", "table", "max_n"]
    sig = inspect.signature(c.attend_paged_packed)
    assert list(sig.parameters) == ["self", "Q", "cu", "lens", "table", "max_nq", "out"] and sig.parameters["out"].default is None


def test_compiled_module_has_the_methods(lib):
    import sys
    from quantizedmha_amd import _lib
    sys.path.insert(0, _lib.LIB_DIR)
    try:
        import torch_ext
    finally:
        sys.path.pop(0)
    i = r"(int|typing\.SupportsInt)"  # how the pybind11 at hand spells an int64_t argument
    t, opt = r"torch\.Tensor", r"(Optional\[torch\.Tensor\]|torch\.Tensor \| None)"
    for c in (torch_ext.KVCache, torch_ext.GroupedKVCache):
        doc = c.append_packed.__doc__
        assert re.search(rf"append_packed\(self: [\w.]*KVCache, K: {t}, V: {t}, cu: {t}, pos: {t}, max_n: {i}\) -> None", doc), doc
        doc = c.attend_packed.__doc__
        assert re.search(rf"attend_packed\(self: [\w.]*KVCache, Q: {t}, cu: {t}, lens: {t}, max_nq: {i}, out: {opt} = None\) -> {t}", doc), doc
    c = torch_ext.PagedKVCache
    doc = c.append_paged_packed.__doc__
    assert re.search(rf"append_paged_packed\(self: [\w.]*PagedKVCache, K: {t}, V: {t}, cu: {t}, pos: {t}, table: {t}, max_n: {i}\) -> None",
                     doc), doc
    doc = c.attend_paged_packed.__doc__
    assert re.search(rf"attend_paged_packed\(self: [\w.]*PagedKVCache, Q: {t}, cu: {t}, lens: {t}, table: {t}, max_nq: {i}, "
                     rf"out: {opt} = None\) -> {t}", doc), doc


# ---- the restated index arithmetic is the source's -------------------------------------------------------------------------
def test_the_restated_formulas_stand_in_the_source():
    """tests/packed_ref.py restates these lines; a change of one of them must come with a change of the restatement."""
    def lines(name):
        return {ln.strip() for ln in open(os.path.join(CSRC, name)).read().splitlines()}
    for name, wanted in (
            ("qmha_fa_masked.hpp", (
                "__host__ __device__ int max_units() const { return G * ((Nq + 2 * QMHA_GROUP - 2) / QMHA_GROUP); }",
                "v.s = (L - Nq) & (QMHA_GROUP - 1);",
                "const int Lp = (L + QMHA_GROUP - 1) & ~(QMHA_GROUP - 1), Nqp = (v.s + Nq + QMHA_GROUP - 1) & ~(QMHA_GROUP - 1);",
                "v.GL = Lp / QMHA_GROUP;  // <= Gk: cap is a multiple of 32",
                "v.Ga = Nqp / QMHA_GROUP;",
                "v.diag_off = (Lp - Nqp) / QMHA_GROUP;",
                "__device__ int last(int g) const { return min(g + diag_off, GL - 1); }",
                "__host__ __device__ int units() const { return G * Ga; }",
                "static int masked_nqb(int units) { return (units + kWaves - 1) / kWaves; }  // unit blocks per K/V slice",
                "v.Nq = nq;",
                "static_cast<Base&>(v) = static_cast<const Base&>(v).of(L);",
                "v.row0 = first;",
                "__device__ __forceinline__ bool row_real(const Packed<Geo>& g, int row) { return (unsigned)(row - g.s) < (unsigned)g.Nq; }",
                "__device__ __forceinline__ int row_shift(const Packed<Geo>& g) { return g.s; }",
                "__device__ __forceinline__ size_t seq_row0(const Packed<Geo>& g, int) { return (size_t)g.row0; }",
                "const int r0 = __builtin_amdgcn_readfirstlane(any.cu[b]), r1 = __builtin_amdgcn_readfirstlane(any.cu[b + 1]);",
                "if (r0 < 0 || r1 < r0 || r1 > any.total) return q;  // the range never becomes an address",
                "if (r1 == r0) return q;                             // an empty sequence sits out",
                "q.row0 = r0, q.nq = r1 - r0, q.verdict = 1;",
                "if (q.nq > any.Nq) return q;  // beyond what the grid was sized for",
                "if (q.L < q.nq || q.L > any.Nk) return q;",
                "if (!any.used_pages_ok(b, q.L)) return q;",
                "if constexpr (kPackedGeo<Geo>) return any.of(q.row0, q.nq, q.L);",
                "float* o = O + (size_t)q.row0 * d_model + (size_t)kvh * G * D;")),
            ("qmha_fa_packed.hip", (
                "const int nqb = masked_nqb(grid_units(geo));",)),
            ("qmha_fa_masked_int8.inc", (
                "if constexpr (kPackedGeo<decltype(geo)>) qrow = Qf + (seq_row0(geo, b) + (size_t)qg * QMHA_GROUP + col) * d_model + (size_t)k * D;",
                "if constexpr (kPackedGeo<decltype(geo)>) orow = O + (seq_row0(geo, b) + (size_t)qg * QMHA_GROUP + col) * d_model + (size_t)k * D + 4 * half;",
                "if (qb * WAVES >= U) continue;          // active unit leaves before any barrier or DMA issue (workgroup-uniform)")),
            ("qmha_fa_masked_f16.inc", (
                "const float* qp = Qf + (seq_row0(geo, b) + (size_t)qg * QMHA_GROUP + 16 * qb + r16 - row_shift(geo)) * d_model + (size_t)k * D +",
                "if (qb0 * WAVES >= U) return;           // no active unit leaves before any barrier or DMA issue")),
            ("qmha_prepass.hip", (
                "static int token_items(int n) { return n <= 2 ? 1 : (n + QMHA_GROUP - 2) / QMHA_GROUP; }",
                "if (c0 < 0 || c1 < c0 || c1 > rows) return false;",
                "const int n = c1 - c0;",
                "if (n == 0 || n > max_n) return false;",
                "return n_b = n, row0 = c0, true;",
                "if (!src.rows_of(b, r.n, r.row0)) return r;",
                "if (p < 0 || p > cap - n) return r;",
                "it.g0 = p / QMHA_GROUP, it.g1 = (p + n - 1) / QMHA_GROUP;",
                "if (it.j == 0 || it.j < it.g1 - it.g0) it.p = p;",
                "const int lo = p - g * QMHA_GROUP, hi = lo + n;  // the new rows of this group: lo <= r < hi",
                "const size_t src = r.row0 * d_model + col, trow = (size_t)b * QMHA_GROUP * d_model + col;",
                "const int maxg = token_items(max_n), total = B * H * maxg;"))):
        have = lines(name)
        for ln in wanted:
            assert ln in have, (name, ln)


# ---- the sweeps --------------------------------------------------------------------------------------------------------------
SWEEP_CAP = 224


@pytest.mark.parametrize("max_nq", [1, 5, 32, 40])
def test_attend_prologue_sweep(max_nq):
    """cap = 224, every nq_b in [0, max_nq + 1] and every L in [0, cap + 1], the range somewhere inside [0, total)."""
    cap, c0 = SWEEP_CAP, 3
    total = c0 + max_nq + 1 + 2  # two spare rows behind the longest range
    grid_units = pk.max_units(max_nq)
    nqb = pk.nqb_of(grid_units)
    ran = zeroed = skipped = 0
    for nq in range(0, max_nq + 2):
        c1 = c0 + nq
        for L in range(0, cap + 2):
            verdict, row0, n = pk.packed_seq(c0, c1, total, max_nq, L, cap)
            if nq == 0:
                assert verdict == pk.SKIP  # sits out whatever L is
                skipped += 1
                continue
            assert (row0, n) == (c0, nq)
            if nq > max_nq or L < nq or L > cap:
                # an invalid sequence: the only addresses are the zeroed rows of O, its own range
                assert verdict == pk.ZERO and 0 <= row0 and row0 + n <= total and (row0, row0 + n) == (c0, c1)
                zeroed += 1
                continue
            assert verdict == pk.RUN
            ran += 1
            geo = pk.ragged_geo(nq, L)
            # the sequence's active units fit the grid: every active unit block qb has qb < nqb
            assert 1 <= geo["Ga"] <= grid_units and pk.nqb_of(geo["Ga"]) <= nqb, (nq, L, geo)
            assert geo["GL"] <= cap // 32 and geo["diag_off"] >= 0
            # the real rows of the lanes of the active groups are exactly the range, each once
            rows = [pk.lane_row(row0, geo, qg, col) for qg in range(geo["Ga"]) for col in range(32)]
            real = [r for r in rows if r is not None]
            assert real == list(range(c0, c1)), (nq, L)
            # a group of the grid beyond Ga has no real lane (its workgroup leaves, or its wave is inactive)
            assert all(pk.lane_row(row0, geo, qg, col) is None for qg in range(geo["Ga"], grid_units) for col in range(32))
            # every tile a group visits lies in the sequence's ceil32(L) rows, and every group has a tile to visit
            for qg in range(geo["Ga"]):
                assert 0 <= pk.last_tile(geo, qg) <= pk.ceil32(L) // 32 - 1, (nq, L, qg)
            # the last real row's diagonal is the sequence's last tile: row s + nq - 1 sees keys up to L - 1
            assert geo["Ga"] - 1 + geo["diag_off"] == pk.ceil32(L) // 32 - 1
    assert ran > 0 and zeroed > 0 and skipped == cap + 2
    # ranges that are out of bounds never become an address, whatever lens holds
    for c0_, c1_ in ((-1, 3), (5, 4), (total - 1, total + 1), (total + 1, total + 2), (-4, -2), (2 ** 31 - 1, -2 ** 31)):
        for L in (0, 5, cap, cap + 1):
            assert pk.packed_seq(c0_, c1_, total, max_nq, L, cap) == (pk.SKIP, 0, 0)
    # the paged kernels' verdict on a used table entry outside the pool
    assert pk.packed_seq(c0, c0 + 1, total, max_nq, 40, cap, pages_ok=False)[0] == pk.ZERO


@pytest.mark.parametrize("max_n", [1, 5, 32, 40])
def test_append_items_sweep(max_n):
    """cap = 224, every n_b in [0, max_n + 1] at every pos in [-1, cap]: the items of the grid cover every touched group once,
    no group lies beyond the cache, every source row lies in the sequence's range and every tail row below 32."""
    cap, c0 = SWEEP_CAP, 3
    rows = c0 + max_n + 1 + 2
    maxg = pk.token_items(max_n)
    for n in range(0, max_n + 2):
        c1 = c0 + n
        for p in range(-1, cap + 1):
            items = [pk.packed_item(c0, c1, rows, max_n, p, cap, j) for j in range(maxg)]
            if n == 0 or n > max_n or p < 0 or p + n > cap:
                assert all(it is None for it in items), (n, p)  # nothing is written, the tail included
                continue
            ran, sources = [], []
            for j, it in enumerate(items):
                if it is None:
                    continue
                nb, row0, g0, g1, groups = it
                assert (nb, row0) == (n, c0)
                for g in groups:
                    assert 0 <= g <= cap // 32 - 1, (n, p, g)
                    new, tail, stays_open = pk.group_rows(p, n, row0, g)
                    assert all(c0 <= src < c1 for src in new.values()) and all(0 <= r < 32 for r in list(new) + tail)
                    assert not tail or g == g0  # only the first group reads the tail
                    assert not stays_open or (j == 0 and g == g1)  # the wave that read the tail is the one that rewrites it
                    sources += sorted(new.values())
                ran += groups
            assert sorted(ran) == list(range(p // 32, (p + n - 1) // 32 + 1)), (n, p, ran)  # every touched group, once
            assert sorted(sources) == list(range(c0, c1)), (n, p)  # every row of the range is placed, once
    for c0_, c1_ in ((-1, 3), (5, 4), (rows - 1, rows + 1), (rows + 1, rows + 2)):
        assert all(pk.packed_item(c0_, c1_, rows, max_n, 0, cap, j) is None for j in range(maxg))
