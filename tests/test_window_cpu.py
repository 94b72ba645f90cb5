"""CPU tests of the sliding-window attends: qmha_attend_cached_tokens_window and
qmha_attend_cached_paged_window.

Every host check of the calls runs before any HIP call, so they are reached here with dummy pointers (as
tests/test_packed_cpu.py does).  The shipped library holds ten windowed kernels under names of their own beside the
kernels it held before.  And the sweep -- tiles first(qg) ... diag(qg) from the zero state, the complementary mask on the
left tile -- is restated in tests/window_ref.py and held here to float64 band attention on the inputs the GPU tests run,
with four private mutants that those inputs catch.
"""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from tests import append_syms

from tests import window_ref as wr
from tests.gpu_support import BUILT, F16, INT8

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAUSAL = 1
V1A, I8 = 1, 2
MEM = 0x10000  # 256-byte aligned, never dereferenced: checks run first
DUMMY = ctypes.c_void_p(0x1000)
B, CAP = 2, 256
NUM_PAGES, PAGE_ROWS, MAX_PAGES = 8, 64, 4  # the paged cache's logical capacity is CAP too
KINDS = {"multi-head": (128, 2, 2, False), "grouped": (256, 4, 2, False), "paged": (256, 4, 2, True)}  # (d_model, h, h_kv, paged), d = 64
NAMES = ("qmha_attend_cached_tokens_window", "qmha_attend_cached_paged_window")


@pytest.fixture(scope="module")
def lib():
    from tools.build import build
    build(verbose=False)
    from quantizedmha_amd import _lib
    return _lib.load()


def make(lib, kind, variant=I8):
    d_model, h, h_kv, pg = KINDS[kind]
    handle = ctypes.c_void_p()
    if pg:
        nbytes = lib.qmha_kv_cache_paged_bytes(NUM_PAGES, PAGE_ROWS, d_model, h, h_kv, variant)
        st = lib.qmha_kv_cache_create_paged(ctypes.byref(handle), ctypes.c_void_p(MEM), nbytes, B, NUM_PAGES, PAGE_ROWS, MAX_PAGES,
                                            d_model, h, h_kv, variant)
    else:
        nbytes = lib.qmha_kv_cache_bytes(B, CAP, h_kv * 64, h_kv, variant)
        st = lib.qmha_kv_cache_create_gqa(ctypes.byref(handle), ctypes.c_void_p(MEM), nbytes, B, CAP, d_model, h, h_kv, variant)
    assert st == 0 and handle.value, (st, lib.qmha_last_error())
    handle.paged = pg
    return handle


@pytest.fixture(params=[(k, v) for k in KINDS for v in (I8, V1A)], ids=lambda p: f"{p[0]}-{'int8' if p[1] == I8 else 'f16'}")
def cache(lib, request):
    handle = make(lib, *request.param)
    yield handle
    lib.qmha_kv_cache_destroy(handle)


def err(lib):
    return lib.qmha_last_error().decode()


def attend(lib, c, Q=DUMMY, O=DUMMY, Nq=4, lens=DUMMY, table=DUMMY, window=64, flags=CAUSAL, paged=None):
    """The windowed entry point of the cache's kind (or of `paged`)."""
    if (c is not None and c.paged) if paged is None else paged:
        return lib.qmha_attend_cached_paged_window(c, Q, O, Nq, lens, table, window, flags, None)
    return lib.qmha_attend_cached_tokens_window(c, Q, O, Nq, lens, window, flags, None)


# ---- 1. the declarations, the exports, the kernels, the bindings (these fail on a library without the feature) -----------
def test_header_declares_the_two_calls():
    header = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "launchers.h")).read())
    for decl in ("int qmha_attend_cached_tokens_window(qmha_kv_cache_t *c, const float *Q, float *O, int Nq, const int32_t *lens, "
                 "int window, unsigned flags, void *stream);",
                 "int qmha_attend_cached_paged_window(qmha_kv_cache_t *c, const float *Q, float *O, int Nq, const int32_t *lens, "
                 "const int32_t *table, int window, unsigned flags, void *stream);"):
        assert decl in header, decl
    for words in ("i + L - Nq - window < j <= i + L - Nq", "a multiple of 32, >= 32", "bit for bit", "[64 * (first(0) / 2), L)",
                  "Columns behind them are not loaded"):
        assert words in header, words


def test_library_exports_the_two_calls(lib):
    from quantizedmha_amd import _lib
    vp, i, u = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint
    for name, argtypes in zip(NAMES, ([vp, vp, vp, i, vp, i, u, vp], [vp, vp, vp, i, vp, vp, i, u, vp])):
        fn = getattr(lib, name)  # AttributeError on a library without the symbol
        assert fn.restype is i and list(fn.argtypes) == argtypes, name
    dyn = subprocess.run(["nm", "-D", "--defined-only", os.path.join(_lib.LIB_DIR, "libqmha.so")], capture_output=True, text=True,
                         check=True).stdout
    for name in NAMES:
        assert re.search(rf" T {name}$", dyn, re.M), name


def test_library_has_the_ten_window_kernels_beside_the_old(lib):
    from quantizedmha_amd import _lib
    syms = subprocess.run(["nm", os.path.join(_lib.LIB_DIR, "libqmha.so")], capture_output=True, text=True, check=True).stdout
    sizes = {"int8": ["128", "32", "64"], "f16": ["128", "64"]}
    want = sorted((f"qmha_fa_{p}_window_kernel", d) for p, ds in sizes.items() for d in ds)
    for base in ("6Ragged", "5Paged"):
        got = sorted(set(re.findall(rf"__device_stub__(qmha_fa_(?:int8|f16)_window_kernel)INS_{base}ELi(\d+)EEEv", syms)))
        assert got == want, (base, got)
    assert len(set(re.findall(r"__device_stub__(qmha_fa_\w+?_window_kernel\w*)", syms))) == 10  # two geometries, nothing else
    # what the library held before
    masked = set(re.findall(r"__device_stub__(qmha_fa_\w+?_masked_kernel)ILi(\d+)ENS_\d+([A-Za-z]+?)E(\w*)", syms))
    assert len(masked) == 15 and {m[2] for m in masked} == {"SquareCausal", "Rect", "Grouped"}, sorted(masked)
    for family, n in ((r"qmha_fa_\w+?_varlen_kernel\w*", 5), (r"qmha_fa_\w+?_cache_kernel\w*", 20),
                      (r"qmha_fa_\w+?_cache_kernelILi\d+ENS_6Ragged\w*", 5), (r"qmha_fa_\w+?_cache_kernelILi\d+ENS_5Paged\w*", 5),
                      (r"qmha_fa_\w+?_cache_kernelILi\d+ENS_6Packed\w*", 10),
                      (r"qmha_fa_\w+?_split_kernelILi\d+ENS_6Ragged\w*", 5), (r"qmha_fa_\w+?_split_kernelILi\d+ENS_5Paged\w*", 5),
                      (r"qmha_split_combine_kernel\w*", 1)):
        assert len(set(re.findall(rf"__device_stub__({family})", syms))) == n, family
    # the appends: five instances of each policy pair of the rows template (token, paged, packed, packed pages) and of each
    # row policy of the append template (append, place)
    for src in append_syms.SRCS:
        for dst in append_syms.DSTS:
            assert append_syms.rows(syms, src=src, dst=dst) == append_syms.want_rows((src,), (dst,)), (src, dst)
    for row in append_syms.ROWS:
        assert append_syms.append(syms, row=row) == append_syms.want_append((row,)), row
    append_syms.check_family(syms)


def test_python_binding_has_the_methods():
    from quantizedmha_amd import torch_ext
    for c in (torch_ext.KVCache, torch_ext.GroupedKVCache):
        sig = inspect.signature(c.attend_tokens_window)
        assert list(sig.parameters) == ["self", "Q", "lens", "window", "out"] and sig.parameters["out"].default is None
        assert list(inspect.signature(c.attend_tokens).parameters) == ["self", "Q", "lens", "out"]  # unchanged
    sig = inspect.signature(torch_ext.PagedKVCache.attend_paged_window)
    assert list(sig.parameters) == ["self", "Q", "lens", "table", "window", "out"] and sig.parameters["out"].default is None
    assert list(inspect.signature(torch_ext.PagedKVCache.attend_paged).parameters) == ["self", "Q", "lens", "table", "out"]


def test_compiled_module_has_the_methods(lib):
    from tests.gpu_support import compiled_module
    torch_ext = compiled_module()
    i = r"(int|typing\.SupportsInt)"  # how the pybind11 at hand spells an int64_t argument
    t, opt = r"torch\.Tensor", r"(Optional\[torch\.Tensor\]|torch\.Tensor \| None)"
    for c in (torch_ext.KVCache, torch_ext.GroupedKVCache):
        doc = c.attend_tokens_window.__doc__
        assert re.search(rf"attend_tokens_window\(self: [\w.]*KVCache, Q: {t}, lens: {t}, window: {i}, out: {opt} = None\) -> {t}", doc), doc
    doc = torch_ext.PagedKVCache.attend_paged_window.__doc__
    assert re.search(rf"attend_paged_window\(self: [\w.]*PagedKVCache, Q: {t}, lens: {t}, table: {t}, window: {i}, "
                     rf"out: {opt} = None\) -> {t}", doc), doc


# ---- 2. the calls' host rejections ---------------------------------------------------------------------------------------
def test_window_rejections(lib, cache):
    for window in (0, -32, -1, 31, 48, 33, 2 ** 31 - 1):
        st = attend(lib, cache, window=window)
        assert st == 1 and f"window = {window} rows" in err(lib) and "multiple of 32 with window >= 32" in err(lib), (window, st, err(lib))
    name = "attend_paged_window" if cache.paged else "attend_tokens_window"
    assert attend(lib, cache, window=48) == 1 and err(lib).startswith(name + ": "), err(lib)
    for flags in (0, 2, 3, 0x80000001):
        assert attend(lib, cache, flags=flags) == 1 and "must be QMHA_FLAG_CAUSAL" in err(lib), (flags, err(lib))
    for kw, cause in (({"Q": None}, "null tensor"), ({"O": None}, "null tensor"), ({"lens": None}, "null lens")):
        assert attend(lib, cache, **kw) == 1 and cause in err(lib), (kw, err(lib))
    if cache.paged:
        assert attend(lib, cache, table=None) == 1 and "null table" in err(lib)
    for Nq in (0, -1, CAP + 1):
        st = attend(lib, cache, Nq=Nq)
        assert st == 1 and f"Nq = {Nq} rows, needs 1 <= Nq <= cap" in err(lib), (Nq, st, err(lib))
    # the unwindowed call's checks come first, in their order: a bad Nq wins over a bad window, flags over both
    assert attend(lib, cache, Nq=0, window=48) == 1 and "Nq = 0" in err(lib)
    assert attend(lib, cache, Nq=0, window=48, flags=0) == 1 and "QMHA_FLAG_CAUSAL" in err(lib)
    assert attend(lib, None, paged=False) == 1 and "null cache" in err(lib)
    assert attend(lib, None, paged=True) == 1 and "null cache" in err(lib)
    cause = "the cache is paged" if cache.paged else "the cache is contiguous"
    assert attend(lib, cache, paged=not cache.paged) == 1 and cause in err(lib), err(lib)


def test_an_int8_cache_needs_what_attend_tokens_needs(lib, cache):
    """attend_tokens asks nothing of an int8 cache beyond the cache itself (the tail belongs to the appends): with and without
    an attached tail the windowed call gives attend_tokens' verdict on the same arguments."""
    def plain(**kw):
        if cache.paged:
            return lib.qmha_attend_cached_paged(cache, DUMMY, DUMMY, kw.get("Nq", 4), DUMMY, DUMMY, kw.get("flags", CAUSAL), None)
        return lib.qmha_attend_cached_tokens(cache, DUMMY, DUMMY, kw.get("Nq", 4), DUMMY, kw.get("flags", CAUSAL), None)
    for kw in ({"Nq": 0}, {"flags": 0}, {"Nq": CAP + 1}):
        st0 = plain(**kw)
        e0 = err(lib).split(": ", 1)[1]
        assert attend(lib, cache, **kw) == st0 == 1 and err(lib).split(": ", 1)[1] == e0, (kw, e0, err(lib))


def has_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except ImportError:
        return False


@pytest.mark.skipif(has_gpu(), reason="needs a machine without a GPU: the launch itself must fail")
def test_calls_that_pass_the_checks_reach_the_launch(lib, cache):
    for Nq, window in ((1, 32), (5, 64), (CAP, 96), (40, CAP), (1, 2 ** 31 - 32)):
        assert attend(lib, cache, Nq=Nq, window=window) == 2, err(lib)


# ---- 3. the restatement against float64, 4. the mutants, 5. a window that covers the sequence ------------------------------
@pytest.fixture(scope="module")
def f64_cases():
    return wr.float64_inputs(tuple(BUILT))


WORST = {}


@pytest.mark.parametrize("variant,d", BUILT)
def test_restatement_is_within_the_bounds_of_float64(oracle_mod, f64_cases, variant, d):
    """DESIGN.md 17.1's bounds (int8 5e-3, fp16 max(1e-3, 1e-3 |ref|)) over the real rows, at window 64 and 96: every row of
    these shapes sees min(window, 33 or more) keys, which is enough for the int8 bound on the project's distributions."""
    ran, worst = 0, 0.0
    for label, v, dd, h, h_kv, window, lens, Nq, Q, K, V in f64_cases:
        if (v, dd) != (variant, d):
            continue
        for b, L in enumerate(lens):
            got, _ = wr.attend(oracle_mod, variant, Q[b], K[b], V[b], L, h, h_kv, window)
            ref = wr.attention_f64(Q[b], K[b], V[b], L, h, h_kv, window)
            e = float(np.abs(got - ref).max())
            worst = max(worst, e)
            assert wr.within_bound(variant, got, ref), (label, b, e)
            assert int(wr.keys_seen(L, Nq, window).min()) >= 33
        ran += 1
    print(f"{variant} d{d}: worst |restatement - float64| = {worst:.3e} over {ran} cases")
    assert ran >= 12


@pytest.mark.parametrize("mutant", wr.MUTANTS)
@pytest.mark.parametrize("variant,d", BUILT)
def test_each_mutant_leaves_the_bounds(oracle_mod, f64_cases, variant, d, mutant):
    """On the multi-head normal inputs of the float64 test.  A mutant can show only on a sequence whose window cuts something:
    some group with diag - w >= 0 (first_off_by_one, no_left_mask, left_mask_inclusive change the left tile, which exists
    only then) or diag - w >= 1 (sweep_from_zero_tile adds the tiles before first, of which there are none otherwise).  On
    every case, some sequence with such a group must leave the bound, and the sequences without one must be untouched."""
    shown = 0
    for label, v, dd, h, h_kv, window, lens, Nq, Q, K, V in f64_cases:
        if (v, dd) != (variant, d) or h != h_kv or " normal " not in label:
            continue
        caught = []
        for b, L in enumerate(lens):
            s, Nqp, Lp, off, w = wr.geometry(L, Nq, window)
            need = 1 if mutant == "sweep_from_zero_tile" else 0
            can_show = Nqp // 32 - 1 + off - w >= need
            ref = wr.attention_f64(Q[b], K[b], V[b], L, h, h_kv, window)
            good, _ = wr.attend(oracle_mod, variant, Q[b], K[b], V[b], L, h, h_kv, window)
            got, _ = wr.attend(oracle_mod, variant, Q[b], K[b], V[b], L, h, h_kv, window, mutant=mutant)
            if not can_show:
                assert np.array_equal(got, good), (label, b, mutant)
                continue
            caught.append(not wr.within_bound(variant, got, ref))
        assert caught and any(caught), (label, mutant, caught)
        shown += 1
    assert shown >= 4


@pytest.mark.parametrize("variant,d", BUILT)
def test_a_window_that_covers_the_sequence_is_the_unwindowed_restatement(oracle_mod, variant, d):
    Q, K, V = wr.random_inputs(d, 2, 2, 40, "normal", 9990 + d)
    for lens, Nq in (([33, 95, 224], 5), ([1, 64, 193], 1), ([40, 100, 224], 40)):
        for b, L in enumerate(lens):
            want, _ = wr.attend(oracle_mod, variant, Q[b, :Nq], K[b], V[b], L, 2, 2, 32, unwindowed=True)
            for window in (wr.ceil32(L), wr.ceil32(L) + 32, 2 ** 31 - 32):
                got, _ = wr.attend(oracle_mod, variant, Q[b, :Nq], K[b], V[b], L, 2, 2, window)
                assert np.array_equal(got, want), (lens, Nq, b, window)
            if L > 64:  # and a window that cuts something is another function
                assert not np.array_equal(wr.attend(oracle_mod, variant, Q[b, :Nq], K[b], V[b], L, 2, 2, 32)[0], want)
