"""CPU tests of the split-KV attend: qmha_attend_split_bytes, qmha_attend_cached_tokens_split and
qmha_attend_cached_paged_split.

Every host check of the calls runs before any HIP call, so they are reached here with dummy pointers (as
tests/test_paged_cpu.py does).  The shipped library holds ten split main kernels and one combine kernel under names of
their own, beside the kernels it held before.  And the contract -- chunks of the key sweep from the zero state, joined
with log-sum-exp weights in fp32 -- is restated in numpy (tests/split_ref.py) and held to float64 at the bounds of
DESIGN.md 17.1, with private mutants of the combine that the inputs of tests/test_gpu_split.py are shown to catch.
"""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from tests import append_syms

from tests import split_ref as sr
from tests.gpu_support import BUILT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAUSAL = 1
V1A, INT8 = 1, 2
MEM = 0x10000  # 256-byte aligned, never dereferenced: checks run first
DUMMY = ctypes.c_void_p(0x1000)
B, CAP = 2, 256
# (d_model, h, h_kv) at d = 64; "paged": pages of 64 rows, max_pages = 4
KINDS = {"multi-head": (128, 2, 2), "grouped": (256, 4, 2), "paged": (256, 4, 2)}


@pytest.fixture(scope="module")
def lib():
    from tools.build import build
    build(verbose=False)
    from quantizedmha_amd import _lib
    return _lib.load()


def make_cache(lib, kind, variant=INT8):
    d_model, h, h_kv = KINDS[kind]
    handle = ctypes.c_void_p()
    if kind == "paged":
        nbytes = lib.qmha_kv_cache_paged_bytes(8, 64, d_model, h, h_kv, variant)
        st = lib.qmha_kv_cache_create_paged(ctypes.byref(handle), ctypes.c_void_p(MEM), nbytes, B, 8, 64, CAP // 64, d_model, h, h_kv, variant)
    else:
        nbytes = lib.qmha_kv_cache_bytes(B, CAP, h_kv * 64, h_kv, variant)
        st = lib.qmha_kv_cache_create_gqa(ctypes.byref(handle), ctypes.c_void_p(MEM), nbytes, B, CAP, d_model, h, h_kv, variant)
    assert st == 0 and handle.value, (st, lib.qmha_last_error())
    return handle


@pytest.fixture(params=list(KINDS))
def cache(lib, request):
    handle = make_cache(lib, request.param)
    yield request.param, handle
    lib.qmha_kv_cache_destroy(handle)


def err(lib):
    return lib.qmha_last_error().decode()


def split_call(lib, kind, handle, Q=DUMMY, O=DUMMY, Nq=1, lens=DUMMY, table=DUMMY, chunk=64, scratch=MEM, nbytes=None, flags=CAUSAL):
    """The entry point of the cache's kind; nbytes None: what qmha_attend_split_bytes asks for."""
    if nbytes is None:
        nbytes = lib.qmha_attend_split_bytes(handle, Nq, chunk)
    scratch = ctypes.c_void_p(scratch) if scratch else None
    if kind == "paged":
        return lib.qmha_attend_cached_paged_split(handle, Q, O, Nq, lens, table, chunk, scratch, nbytes, flags, None)
    return lib.qmha_attend_cached_tokens_split(handle, Q, O, Nq, lens, chunk, scratch, nbytes, flags, None)


# ---- the declarations and the exports (these fail on a library without the feature) -------------------------------------
def test_header_declares_the_three_calls():
    header = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "launchers.h")).read())
    for decl in ("size_t qmha_attend_split_bytes(const qmha_kv_cache_t *c, int Nq, int chunk_rows);",
                 "int qmha_attend_cached_tokens_split(qmha_kv_cache_t *c, const float *Q, float *O, int Nq, const int32_t *lens, "
                 "int chunk_rows, void *scratch, size_t scratch_bytes, unsigned flags, void *stream);",
                 "int qmha_attend_cached_paged_split(qmha_kv_cache_t *c, const float *Q, float *O, int Nq, const int32_t *lens, "
                 "const int32_t *table, int chunk_rows, void *scratch, size_t scratch_bytes, unsigned flags, void *stream);"):
        assert decl in header, decl
    # the header documents the scratch layout
    assert "Oc [B][NC][Nq][h * d]" in header and "m [B][NC][Nq][h]" in header and "l [B][NC][Nq][h]" in header


def test_library_exports_the_three_calls(lib):
    from quantizedmha_amd import _lib
    vp, i, sz, u = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_uint
    for name, res, argtypes in (("qmha_attend_split_bytes", sz, [vp, i, i]),
                                ("qmha_attend_cached_tokens_split", i, [vp, vp, vp, i, vp, i, vp, sz, u, vp]),
                                ("qmha_attend_cached_paged_split", i, [vp, vp, vp, i, vp, vp, i, vp, sz, u, vp])):
        fn = getattr(lib, name)  # AttributeError on a library without the symbol
        assert fn.restype is res and list(fn.argtypes) == argtypes, name
    path = os.path.join(_lib.LIB_DIR, "libqmha.so")
    dyn = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    for name in ("qmha_attend_split_bytes", "qmha_attend_cached_tokens_split", "qmha_attend_cached_paged_split"):
        assert re.search(rf" T {name}$", dyn, re.M), name


# ---- the scratch ------------------------------------------------------------------------------------------------------
def test_split_bytes_is_the_documented_layout(lib, cache):
    kind, handle = cache
    d_model, h, _ = KINDS[kind]
    al = lambda x: -(-x // 256) * 256  # noqa: E731
    for Nq, chunk in ((1, 64), (1, 128), (5, 64), (32, 192), (40, 256), (CAP, 64)):
        rows = B * -(-CAP // chunk) * Nq
        assert lib.qmha_attend_split_bytes(handle, Nq, chunk) == al(4 * rows * d_model) + 2 * al(4 * rows * h), (Nq, chunk)
    for Nq, chunk in ((0, 64), (-1, 64), (CAP + 1, 64), (1, 0), (1, 32), (1, 96), (1, 100), (1, -64), (1, CAP + 64)):
        assert lib.qmha_attend_split_bytes(handle, Nq, chunk) == 0, (Nq, chunk)
    assert lib.qmha_attend_split_bytes(None, 1, 64) == 0


# ---- the calls' host rejections ------------------------------------------------------------------------------------------
def test_split_rejections(lib, cache):
    kind, handle = cache
    what = "attend_paged_split" if kind == "paged" else "attend_tokens_split"
    for Nq, flags, cause in ((1, 0, "must be QMHA_FLAG_CAUSAL"), (32, 2, "must be QMHA_FLAG_CAUSAL"), (5, 3, "must be QMHA_FLAG_CAUSAL"),
                             (1, 0x80000001, "must be QMHA_FLAG_CAUSAL"), (0, CAUSAL, "1 <= Nq <= cap"), (-5, CAUSAL, "1 <= Nq <= cap"),
                             (CAP + 1, CAUSAL, "1 <= Nq <= cap")):
        st = split_call(lib, kind, handle, Nq=Nq, flags=flags, nbytes=1 << 30)
        assert st == 1 and cause in err(lib) and what in err(lib), (Nq, flags, st, err(lib))
    for chunk in (0, 32, 96, 100, -64, CAP + 64, 63):
        st = split_call(lib, kind, handle, chunk=chunk, nbytes=1 << 30)
        assert st == 1 and "chunk_rows" in err(lib) and "multiple of 64" in err(lib), (chunk, st, err(lib))
    assert split_call(lib, kind, handle, Q=None) == 1 and "null tensor" in err(lib)
    assert split_call(lib, kind, handle, O=None) == 1 and "null tensor" in err(lib)
    assert split_call(lib, kind, handle, lens=None) == 1 and "null lens" in err(lib)
    if kind == "paged":
        assert split_call(lib, kind, handle, table=None) == 1 and "null table" in err(lib)
    assert split_call(lib, kind, handle, scratch=None) == 1 and "null scratch" in err(lib)
    assert split_call(lib, kind, handle, scratch=MEM + 64) == 1 and "256-byte aligned" in err(lib)
    for Nq, chunk in ((1, 64), (5, 128), (40, 256)):
        need = lib.qmha_attend_split_bytes(handle, Nq, chunk)
        for nbytes in (0, need - 1):
            st = split_call(lib, kind, handle, Nq=Nq, chunk=chunk, nbytes=nbytes)
            assert st == 1 and "scratch too small" in err(lib) and "qmha_attend_split_bytes" in err(lib), (Nq, chunk, nbytes, err(lib))
    assert lib.qmha_attend_cached_tokens_split(None, DUMMY, DUMMY, 1, DUMMY, 64, ctypes.c_void_p(MEM), 1 << 20, CAUSAL, None) == 1
    assert "null cache" in err(lib)
    assert lib.qmha_attend_cached_paged_split(None, DUMMY, DUMMY, 1, DUMMY, DUMMY, 64, ctypes.c_void_p(MEM), 1 << 20, CAUSAL, None) == 1
    assert "null cache" in err(lib)


def test_each_entry_point_refuses_the_other_kind_of_cache(lib, cache):
    kind, handle = cache
    scratch, nbytes = ctypes.c_void_p(MEM), lib.qmha_attend_split_bytes(handle, 1, 64)
    if kind == "paged":
        st = lib.qmha_attend_cached_tokens_split(handle, DUMMY, DUMMY, 1, DUMMY, 64, scratch, nbytes, CAUSAL, None)
        assert st == 1 and "the cache is paged" in err(lib), err(lib)
    else:
        st = lib.qmha_attend_cached_paged_split(handle, DUMMY, DUMMY, 1, DUMMY, DUMMY, 64, scratch, nbytes, CAUSAL, None)
        assert st == 1 and "the cache is contiguous" in err(lib), err(lib)


def has_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except ImportError:
        return False


@pytest.mark.skipif(has_gpu(), reason="needs a machine without a GPU: the launch itself must fail")
def test_calls_that_pass_the_checks_reach_the_launch(lib, cache):
    kind, handle = cache
    for Nq, chunk in ((1, 64), (5, 128), (40, 64), (CAP, CAP)):
        assert split_call(lib, kind, handle, Nq=Nq, chunk=chunk) == 2, err(lib)


# ---- the kernels ---------------------------------------------------------------------------------------------------------
def test_library_has_the_eleven_split_kernels_beside_the_old(lib):
    path = os.path.join(ROOT, "quantizedmha_amd", "lib", "libqmha.so")
    syms = subprocess.run(["nm", path], capture_output=True, text=True, check=True).stdout
    # one split template per precision, over Ragged and over Paged
    main = sorted(set(re.findall(r"__device_stub__(qmha_fa_(?:int8|f16)_split_kernel)ILi(\d+)ENS_\d+(Ragged|Paged)EEEv", syms)))
    stem = lambda v: "int8" if v == "fa_tc_int8_b" else "f16"  # noqa: E731
    want = sorted([(f"qmha_fa_{stem(v)}_split_kernel", str(d), "Ragged") for v, d in BUILT] +
                  [(f"qmha_fa_{stem(v)}_split_kernel", str(d), "Paged") for v, d in BUILT])
    assert main == want and len(main) == 10, main
    # one instance of each per head size: no third geometry, no dumping twin
    assert len(set(re.findall(r"__device_stub__(qmha_fa_\w+?_split_kernelILi\d+ENS_6Ragged\w*)", syms))) == 5
    assert len(set(re.findall(r"__device_stub__(qmha_fa_\w+?_split_kernelILi\d+ENS_5Paged\w*)", syms))) == 5
    assert len(set(re.findall(r"__device_stub__(qmha_fa_\w+?_split\w*_kernel\w*)", syms))) == 10
    assert len(set(re.findall(r"__device_stub__(qmha_split_combine_kernel\w*)", syms))) == 1
    # what the library held before
    masked = set(re.findall(r"__device_stub__(qmha_fa_\w+?_masked_kernel)ILi(\d+)ENS_\d+([A-Za-z]+?)E(\w*)", syms))
    assert len(masked) == 15 and {m[2] for m in masked} == {"SquareCausal", "Rect", "Grouped"}, sorted(masked)
    assert len(set(re.findall(r"__device_stub__(qmha_fa_\w+?_varlen_kernel\w*)", syms))) == 5
    assert len(set(re.findall(r"__device_stub__(qmha_fa_\w+?_cache_kernelILi\d+ENS_6Ragged\w*)", syms))) == 5
    assert len(set(re.findall(r"__device_stub__(qmha_fa_\w+?_cache_kernelILi\d+ENS_5Paged\w*)", syms))) == 5
    assert append_syms.rows(syms, src="UniformRows", dst="ContiguousRows") == append_syms.want_rows(("UniformRows",), ("ContiguousRows",))
    assert append_syms.rows(syms, src="UniformRows", dst="PagedTable") == append_syms.want_rows(("UniformRows",), ("PagedTable",))
    append_syms.check_family(syms)


# ---- the bindings ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", ["KVCache", "GroupedKVCache", "PagedKVCache"])
def test_python_binding_has_the_methods(cls):
    from quantizedmha_amd import torch_ext
    c = getattr(torch_ext, cls)
    sig = inspect.signature(c.enable_split)
    assert list(sig.parameters) == ["self", "chunk_rows", "max_nq"] and sig.parameters["max_nq"].default == 32
    assert list(inspect.signature(c.split_partials).parameters) == ["self", "Nq"]
    if cls == "PagedKVCache":
        sig = inspect.signature(c.attend_paged_split)
        assert list(sig.parameters) == ["self", "Q", "lens", "table", "out"] and sig.parameters["out"].default is None
        assert not hasattr(c, "attend_tokens_split")
    else:
        sig = inspect.signature(c.attend_tokens_split)
        assert list(sig.parameters) == ["self", "Q", "lens", "out"] and sig.parameters["out"].default is None
    # the signatures the class had stay as they were
    assert list(inspect.signature(c.enable_tokens).parameters) == ["self"]


@pytest.mark.parametrize("cls", ["KVCache", "GroupedKVCache", "PagedKVCache"])
def test_compiled_module_has_the_methods(lib, cls):
    from tests.gpu_support import compiled_module
    c = getattr(compiled_module(), cls)
    i = r"(int|typing\.SupportsInt)"  # how the pybind11 at hand spells an int64_t argument
    out = r"out: (Optional\[torch\.Tensor\]|torch\.Tensor \| None) = None\) -> torch\.Tensor"
    assert re.search(rf"enable_split\(self: [\w.]*KVCache, chunk_rows: {i}, max_nq: {i} = 32\) -> None", c.enable_split.__doc__), \
        c.enable_split.__doc__
    assert re.search(rf"split_partials\(self: [\w.]*KVCache, Nq: {i}\) -> (tuple|Tuple)\[torch\.Tensor, torch\.Tensor, torch\.Tensor\]",
                     c.split_partials.__doc__), c.split_partials.__doc__
    if cls == "PagedKVCache":
        doc = c.attend_paged_split.__doc__
        assert re.search(r"attend_paged_split\(self: [\w.]*PagedKVCache, Q: torch\.Tensor, lens: torch\.Tensor, table: torch\.Tensor, " + out,
                         doc), doc
    else:
        doc = c.attend_tokens_split.__doc__
        assert re.search(r"attend_tokens_split\(self: [\w.]*KVCache, Q: torch\.Tensor, lens: torch\.Tensor, " + out, doc), doc
    assert hasattr(c, "split_scratch")


# ---- the contract against float64 ----------------------------------------------------------------------------------------
# (cap, L, Nq): every row sees at least 33 keys (tests/test_tokens_cpu.py says why the 5e-3 is asked of such rows only);
# decode steps in a middle and in the last group, short blocks, Nq = 32 at s != 0 (two query groups whose last chunks
# differ at chunk_rows = 64), a partial last chunk (cap 224) and a full one (cap 256)
CONTRACT = [(224, 95, 1), (224, 193, 5), (224, 224, 1), (224, 100, 32), (224, 224, 40), (256, 256, 5), (256, 161, 32)]


@pytest.mark.parametrize("chunk", sr.CHUNKS)
@pytest.mark.parametrize("dist", ["normal", "uniform"])
@pytest.mark.parametrize("variant,d", BUILT)
def test_restatement_against_float64(oracle_mod, variant, d, dist, chunk):
    """The split contract, restated, within int8 5e-3 / fp16 max(1e-3, 1e-3 |ref|) of float64 attention."""
    from tests import rect_ref as rr
    h = 2
    worst = 0.0
    for cap, L, Nq in CONTRACT:
        Q, K, V = rr.inputs(Nq, cap, h * d, 1, dist, 9300 + L + 7 * Nq + d + (1 if dist == "uniform" else 0))
        got = sr.attend(oracle_mod, variant, Q[0], K[0], V[0], L, h, h, chunk, cap)
        ref = sr.attention_f64(Q[0], K[0], V[0], L, h, h)
        e = float(np.abs(got - ref).max())
        worst = max(worst, e)
        print(f"{variant} d{d} {dist} chunk{chunk} cap{cap} L{L} Nq{Nq}: max|split contract - float64| = {e:.2e}")
        assert sr.within_bound(variant, got, ref), (cap, L, Nq, e)
    print(f"{variant} d{d} {dist} chunk{chunk}: worst {worst:.2e}")


def test_grouped_restatement_against_float64(oracle_mod):
    """h = 4 query heads on h_kv = 2 and 1 K/V heads: query head k reads K/V head k // G."""
    from tests import rect_ref as rr
    for variant, d in ((sr.INT8, 64), (sr.F16, 64)):
        for h_kv in (2, 1):
            Q, K, V = rr.inputs(5, 224, 4 * d, 1, "normal", 9400 + h_kv)
            K, V = K[0, :, :h_kv * d], V[0, :, :h_kv * d]
            got = sr.attend(oracle_mod, variant, Q[0], K, V, 193, 4, h_kv, 64, 224)
            assert sr.within_bound(variant, got, sr.attention_f64(Q[0], K, V, 193, 4, h_kv)), (variant, h_kv)


def test_scratch_is_written_where_it_is_read_and_nowhere_else(oracle_mod):
    """The partials over a NaN scratch: finite exactly at the chunks c <= last(qg) // C of each real row."""
    for L, Nq, chunk in ((100, 32, 64), (224, 40, 128), (33, 1, 64), (193, 5, 64)):
        Q, K, V = sr.random_inputs(64, 2, 2, Nq, "normal", 5)
        Oc, pm, pl = sr.partials(oracle_mod, sr.F16, Q[0], K[0], V[0], L, 2, 2, chunk, sr.CAP)
        reads = sr.chunks_read(L, Nq, chunk)
        for r in range(Nq):
            for c in range(Oc.shape[0]):
                fin = np.isfinite(Oc[c, r]).all() and np.isfinite(pm[c, r]).all() and np.isfinite(pl[c, r]).all()
                nan = np.isnan(Oc[c, r]).all() and np.isnan(pm[c, r]).all() and np.isnan(pl[c, r]).all()
                assert fin if c < reads[r] else nan, (L, Nq, chunk, r, c)
    # Nq = 40 at L = 100 spans three query groups (s = 28) whose last tiles 1, 2, 3 lie on both sides of a chunk boundary
    assert list(sr.chunks_read(100, 40, 64)[[0, 3, 4, 39]]) == [1, 1, 2, 2]


# ---- the inputs of the GPU tests: inside the bounds, and sharp enough to catch a wrong combine ---------------------------
def test_gpu_inputs_stay_inside_the_bounds_and_catch_the_mutants(oracle_mod):
    """Every input of the GPU float64 test keeps the unmutated restatement inside the bounds; drop_chunk and read_beyond
    push it outside on EVERY multi-chunk sequence, no_rescale on the climbing-maxima case and on many of the int8 ones
    (on random inputs the chunks' m lie close together, and fp16 keeps m = 0 in every chunk -- the lazy base never
    moves --, so there no_rescale is the contract)."""
    caught = {m: 0 for m in sr.MUTANTS}
    for label, variant, h, h_kv, chunk, seqs, cap in sr.float64_inputs(BUILT):
        hard = "ramp" in label
        for Q, K, V, L in seqs:
            Oc, pm, pl = sr.partials(oracle_mod, variant, Q, K, V, L, h, h_kv, chunk, cap)
            reads = sr.chunks_read(L, Q.shape[0], chunk)
            ref = sr.attention_f64(Q, K, V, L, h, h_kv)
            assert sr.within_bound(variant, sr.combine(variant, Oc, pm, pl, reads), ref), (label, L)
            if reads.max() < 2:
                continue
            for mutant in ("no_rescale", "drop_chunk", "read_beyond"):
                bad = not sr.within_bound(variant, sr.combine(variant, Oc, pm, pl, reads, mutant), ref)
                caught[mutant] += bad
                if hard or mutant != "no_rescale":
                    assert bad, (label, L, mutant)
        if hard:  # the chunks' maxima climb by more than 48 log2 units
            climb = float((np.nanmax(pm, axis=0) - np.nanmin(pm, axis=0)).min())
            print(f"{label}: m climbs by {climb:.1f} log2 units across chunks")
            assert climb > 48.0, (label, climb)
    assert all(caught[m] > 0 for m in ("no_rescale", "drop_chunk", "read_beyond")), caught


@pytest.mark.parametrize("variant,d,name", sr.HARD_COMBINE)
def test_combine_inputs_catch_a_stale_maximum(oracle_mod, variant, d, name):
    """M cancels between the sums, so a wrong M shows only once a weight overflows: the staircase's chunks climb by more
    than 128 log2 units, the restated combine stays inside the GPU combine test's bound of the float64 formula, and every
    mutant -- stale_max among them -- leaves it."""
    Q, K, V, h = sr.hard_inputs(name, d)
    for chunk in sr.CHUNKS:
        Oc, pm, pl = sr.partials(oracle_mod, variant, Q, K, V, sr.HARD_CAP, h, h, chunk, sr.HARD_CAP)
        reads = sr.chunks_read(sr.HARD_CAP, sr.HARD_NQ, chunk)
        assert float((np.nanmax(pm, axis=0) - np.nanmin(pm, axis=0)).min()) > 128.0
        want, bound = sr.combine_f64(Oc, pm, pl, reads, sr.THR[variant])
        inside = lambda got: bool(np.isfinite(got).all() and (np.abs(got - want) <= bound).all())  # noqa: E731
        assert inside(sr.combine(variant, Oc, pm, pl, reads)), (chunk, "the unmutated combine")
        for mutant in sr.MUTANTS:
            assert not inside(sr.combine(variant, Oc, pm, pl, reads, mutant)), (chunk, mutant)
