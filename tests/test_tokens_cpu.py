"""CPU tests of the token-granular entry points of the K/V cache: qmha_kv_cache_tail_bytes,
qmha_kv_cache_attach_tail, qmha_kv_cache_append_tokens and qmha_attend_cached_tokens.

Every host check of the calls runs before any HIP call, so they are reached here with dummy pointers (as
tests/test_varlen_cpu.py does).  The shipped library holds five ragged main kernels and five token append kernels
under names of their own, beside the kernels it held before.  And the contract itself -- a ragged call IS the
existing call on zero-padded operands -- is held to float64 on the CPU with the restatements of tests/rect_ref.py:
the padding must not cost the accuracy the project's bounds ask for.
"""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from tests import append_syms

from tests import rect_ref as rr

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


def make_cache(lib, kind, variant=INT8):
    """B = 2, cap = 256, h = 2 (grouped: h = 4 on 2 K/V heads), d = 64."""
    handle = ctypes.c_void_p()
    nbytes = lib.qmha_kv_cache_bytes(2, 256, 128, 2, variant)
    if kind == "multi-head":
        st = lib.qmha_kv_cache_create(ctypes.byref(handle), ctypes.c_void_p(MEM), nbytes, 2, 256, 128, 2, variant)
    else:
        st = lib.qmha_kv_cache_create_gqa(ctypes.byref(handle), ctypes.c_void_p(MEM), nbytes, 2, 256, 256, 4, 2, variant)
    assert st == 0 and handle.value, (st, lib.qmha_last_error())
    return handle


@pytest.fixture(params=["multi-head", "grouped"])
def cache(lib, request):
    handle = make_cache(lib, request.param)
    yield handle
    lib.qmha_kv_cache_destroy(handle)


TAIL = 2 * 2 * 32 * 2 * 64 * 4  # K and V, B = 2 sequences, 32 rows of h_kv d = 128 fp32


def test_header_declares_the_four_calls():
    header = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "launchers.h")).read())
    for decl in ("size_t qmha_kv_cache_tail_bytes(const qmha_kv_cache_t *c);",
                 "int qmha_kv_cache_attach_tail(qmha_kv_cache_t *c, void *mem, size_t bytes);",
                 "int qmha_kv_cache_append_tokens(qmha_kv_cache_t *c, const float *K, const float *V, int n, const int32_t *pos, "
                 "void *stream);",
                 "int qmha_attend_cached_tokens(qmha_kv_cache_t *c, const float *Q, float *O, int Nq, const int32_t *lens, "
                 "unsigned flags, void *stream);"):
        assert decl in header, decl


def test_library_exports_the_four_calls(lib):
    from quantizedmha_amd import _lib
    vp, i, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
    for name, res, argtypes in (("qmha_kv_cache_tail_bytes", sz, [vp]),
                                ("qmha_kv_cache_attach_tail", i, [vp, vp, sz]),
                                ("qmha_kv_cache_append_tokens", i, [vp, vp, vp, i, vp, vp]),
                                ("qmha_attend_cached_tokens", i, [vp, vp, vp, i, vp, ctypes.c_uint, vp])):
        fn = getattr(lib, name)  # AttributeError on a library without the symbol
        assert fn.restype is res and list(fn.argtypes) == argtypes, name
    path = os.path.join(_lib.LIB_DIR, "libqmha.so")
    dyn = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    for name in ("qmha_kv_cache_tail_bytes", "qmha_kv_cache_attach_tail", "qmha_kv_cache_append_tokens", "qmha_attend_cached_tokens"):
        assert re.search(rf" T {name}$", dyn, re.M), name


def test_tail_size_and_attachment(lib, cache):
    assert lib.qmha_kv_cache_tail_bytes(cache) == TAIL
    assert lib.qmha_kv_cache_tail_bytes(None) == 0
    for mem, nbytes, cause in ((MEM, TAIL - 1, "too small"), (MEM, 0, "too small"), (None, TAIL, "null tail"),
                               (MEM + 64, TAIL, "256-byte aligned")):
        st = lib.qmha_kv_cache_attach_tail(cache, ctypes.c_void_p(mem) if mem else None, nbytes)
        assert st == 1 and cause in lib.qmha_last_error().decode(), (mem, nbytes, st, lib.qmha_last_error())
    assert lib.qmha_kv_cache_attach_tail(None, ctypes.c_void_p(MEM), TAIL) == 1 and "null cache" in lib.qmha_last_error().decode()
    # a refused tail was not attached: the append still asks for one
    st = lib.qmha_kv_cache_append_tokens(cache, DUMMY, DUMMY, 1, DUMMY, None)
    assert st == 1 and "needs its tail" in lib.qmha_last_error().decode(), (st, lib.qmha_last_error())
    assert lib.qmha_kv_cache_attach_tail(cache, ctypes.c_void_p(MEM), TAIL) == 0, lib.qmha_last_error()
    # the cache memory's size is what it was
    assert lib.qmha_kv_cache_bytes(2, 256, 128, 2, INT8) == lib.qmha_workspace_size(2, 256, 128, 2, INT8)


@pytest.mark.parametrize("kind", ["multi-head", "grouped"])
def test_an_fp16_cache_needs_no_tail(lib, kind):
    c = make_cache(lib, kind, V1A)
    try:
        assert lib.qmha_kv_cache_tail_bytes(c) == 0
        assert lib.qmha_kv_cache_attach_tail(c, None, 0) == 0, lib.qmha_last_error()
    finally:
        lib.qmha_kv_cache_destroy(c)


def test_append_tokens_rejections_leave_the_length(lib, cache):
    assert lib.qmha_kv_cache_attach_tail(cache, ctypes.c_void_p(MEM), TAIL) == 0
    for n in (0, -1, 257, 288):
        st = lib.qmha_kv_cache_append_tokens(cache, DUMMY, DUMMY, n, DUMMY, None)
        assert st == 1 and "1 <= n <= cap" in lib.qmha_last_error().decode(), (n, st, lib.qmha_last_error())
        assert lib.qmha_kv_cache_len(cache) == 0
    for args, cause in (((None, DUMMY, 1, DUMMY), "null tensor"), ((DUMMY, None, 1, DUMMY), "null tensor"),
                        ((DUMMY, DUMMY, 1, None), "null pos")):
        assert lib.qmha_kv_cache_append_tokens(cache, *args, None) == 1 and cause in lib.qmha_last_error().decode(), args
        assert lib.qmha_kv_cache_len(cache) == 0
    assert lib.qmha_kv_cache_append_tokens(None, DUMMY, DUMMY, 1, DUMMY, None) == 1 and "null cache" in lib.qmha_last_error().decode()


def test_append_tokens_needs_the_tail_on_an_int8_cache(lib, cache):
    for n in (1, 32, 256):
        st = lib.qmha_kv_cache_append_tokens(cache, DUMMY, DUMMY, n, DUMMY, None)
        assert st == 1 and "needs its tail" in lib.qmha_last_error().decode(), (n, st, lib.qmha_last_error())
    assert lib.qmha_kv_cache_len(cache) == 0


def test_attend_tokens_rejections_leave_the_length(lib, cache):
    for Nq, flags, cause in ((1, 0, "must be QMHA_FLAG_CAUSAL"), (32, 2, "must be QMHA_FLAG_CAUSAL"), (5, 3, "must be QMHA_FLAG_CAUSAL"),
                             (1, 0x80000001, "must be QMHA_FLAG_CAUSAL"), (0, CAUSAL, "1 <= Nq <= cap"),
                             (-5, CAUSAL, "1 <= Nq <= cap"), (257, CAUSAL, "1 <= Nq <= cap")):
        st = lib.qmha_attend_cached_tokens(cache, DUMMY, DUMMY, Nq, DUMMY, flags, None)
        assert st == 1 and cause in lib.qmha_last_error().decode(), (Nq, flags, st, lib.qmha_last_error())
        assert lib.qmha_kv_cache_len(cache) == 0
    for args, cause in (((None, DUMMY, 1, DUMMY), "null tensor"), ((DUMMY, None, 1, DUMMY), "null tensor"),
                        ((DUMMY, DUMMY, 1, None), "null lens")):
        st = lib.qmha_attend_cached_tokens(cache, *args, CAUSAL, None)
        assert st == 1 and cause in lib.qmha_last_error().decode(), (args, lib.qmha_last_error())
    assert lib.qmha_attend_cached_tokens(None, DUMMY, DUMMY, 1, DUMMY, CAUSAL, None) == 1


def has_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except ImportError:
        return False


@pytest.mark.skipif(has_gpu(), reason="needs a machine without a GPU: the launch itself must fail")
def test_calls_that_pass_the_checks_reach_the_launch(lib, cache):
    """Ragged sizes pass the host checks -- the lengths are the device's business -- and get as far as the launch,
    which fails without a device; the host length stays 0."""
    assert lib.qmha_kv_cache_attach_tail(cache, ctypes.c_void_p(MEM), TAIL) == 0
    for n in (1, 33, 256):
        assert lib.qmha_kv_cache_append_tokens(cache, DUMMY, DUMMY, n, DUMMY, None) == 2, lib.qmha_last_error()
    for Nq in (1, 5, 40, 256):
        assert lib.qmha_attend_cached_tokens(cache, DUMMY, DUMMY, Nq, DUMMY, CAUSAL, None) == 2, lib.qmha_last_error()
    assert lib.qmha_kv_cache_len(cache) == 0


def test_library_has_the_ten_new_kernels_beside_the_old(lib):
    path = os.path.join(ROOT, "quantizedmha_amd", "lib", "libqmha.so")
    syms = subprocess.run(["nm", path], capture_output=True, text=True, check=True).stdout
    # the cache kernel template over Ragged (its other geometries: test_paged_cpu.py, test_packed_cpu.py)
    main = sorted(set(re.findall(r"__device_stub__(qmha_fa_(?:int8|f16)_cache_kernel)ILi(\d+)ENS_6RaggedEEEv", syms)))
    assert main == [("qmha_fa_f16_cache_kernel", "128"), ("qmha_fa_f16_cache_kernel", "64"),
                    ("qmha_fa_int8_cache_kernel", "128"), ("qmha_fa_int8_cache_kernel", "32"),
                    ("qmha_fa_int8_cache_kernel", "64")], main
    # the rows template over UniformRows and ContiguousRows (its other policies: test_paged_cpu.py, test_packed_cpu.py)
    token = append_syms.rows(syms, src="UniformRows", dst="ContiguousRows")
    u, c = "UniformRows", "ContiguousRows"
    assert token == [("qmha_kv_rows_f16_kernel", u, c, "128"), ("qmha_kv_rows_f16_kernel", u, c, "64"),
                     ("qmha_kv_rows_int8_kernel", u, c, "128"), ("qmha_kv_rows_int8_kernel", u, c, "32"),
                     ("qmha_kv_rows_int8_kernel", u, c, "64")], token
    # one instance of each: no second geometry, no dumping twin
    assert len(set(re.findall(r"__device_stub__(qmha_fa_\w+?_cache_kernelILi\d+ENS_6Ragged\w*)", syms))) == 5
    assert len(set(re.findall(r"__device_stub__(qmha_fa_\w+?_cache_kernel\w*)", syms))) == 20  # four geometries, nothing else
    append_syms.check_family(syms)  # four policy pairs of the rows template, two of the append template, nothing else
    # what the library held before: fifteen masked and five varlen main kernels, five append and five place kernels
    masked = set(re.findall(r"__device_stub__(qmha_fa_\w+?_masked_kernel)ILi(\d+)ENS_\d+([A-Za-z]+?)E(\w*)", syms))
    assert len(masked) == 15 and {m[2] for m in masked} == {"SquareCausal", "Rect", "Grouped"}, sorted(masked)
    assert len(set(re.findall(r"__device_stub__(qmha_fa_\w+?_varlen_kernel\w*)", syms))) == 5
    assert append_syms.append(syms, row="HostRow") == append_syms.want_append(("HostRow",))
    assert append_syms.append(syms, row="PlacedRow") == append_syms.want_append(("PlacedRow",))


@pytest.mark.parametrize("cls", ["KVCache", "GroupedKVCache"])
def test_python_binding_has_the_three_methods(cls):
    from quantizedmha_amd import torch_ext
    c = getattr(torch_ext, cls)
    assert list(inspect.signature(c.enable_tokens).parameters) == ["self"]
    assert list(inspect.signature(c.append_tokens).parameters) == ["self", "K", "V", "pos"]
    sig = inspect.signature(c.attend_tokens)
    assert list(sig.parameters) == ["self", "Q", "lens", "out"] and sig.parameters["out"].default is None


@pytest.mark.parametrize("cls", ["KVCache", "GroupedKVCache"])
def test_compiled_module_has_the_three_methods(lib, cls):
    import sys
    from quantizedmha_amd import _lib
    sys.path.insert(0, _lib.LIB_DIR)
    try:
        import torch_ext
    finally:
        sys.path.pop(0)
    c = getattr(torch_ext, cls)
    assert re.search(r"enable_tokens\(self: [\w.]*KVCache\) -> None", c.enable_tokens.__doc__), c.enable_tokens.__doc__
    doc = c.append_tokens.__doc__
    assert re.search(r"append_tokens\(self: [\w.]*KVCache, K: torch\.Tensor, V: torch\.Tensor, pos: torch\.Tensor\) -> None", doc), doc
    doc = c.attend_tokens.__doc__
    assert re.search(r"attend_tokens\(self: [\w.]*KVCache, Q: torch\.Tensor, lens: torch\.Tensor, "
                     r"out: (Optional\[torch\.Tensor\]|torch\.Tensor \| None) = None\) -> torch\.Tensor", doc), doc


# ---- the padded contract against float64 --------------------------------------------------------------------------------
def padded_operands(Q, K, V, L):
    """The operands of the existing call that DEFINES the ragged one: Q [B, Nq, m] at rows [s, s + Nq) of
    a zero [B, Nq', m] block, the first L rows of K, V [B, >= L, m] zero-padded to L' = ceil32(L); and s."""
    Nq = Q.shape[1]
    s = (L - Nq) % 32
    Nqp, Lp = -(-(s + Nq) // 32) * 32, -(-L // 32) * 32
    Qp = np.zeros((Q.shape[0], Nqp, Q.shape[2]), np.float32)
    Qp[:, s:s + Nq] = Q
    Kp, Vp = (np.zeros((X.shape[0], Lp, X.shape[2]), np.float32) for X in (K, V))
    Kp[:, :L], Vp[:, :L] = K[:, :L], V[:, :L]
    assert (Lp - Nqp) % 32 == 0 and Lp - Nqp == L - Nq - s
    return Qp, Kp, Vp, s


# (L, Nq): single-token decode in a second, a middle and a last group; short blocks; Nq = 32 at s != 0 (two query
# groups); Nq = 40 at L = 224 (the smaller group count); a long prefill chunk that is no padding at all (s = 0) as the
# yardstick of the yardstick.  Every row here sees at least 33 keys (L - Nq >= 32), as in tests/test_rect_cpu.py: 5e-3
# is a bound for rows that average over keys.  A row that sees ONE key returns that V row as quantised (half a step,
# absmax / 254) times Pi / (127 p) (p < 1 under m0 = 0 when the score is negative: another 1 / (254 p)), which does not
# average out: 7.2e-3 at L = Nq = 1 here -- and 7.6e-3 in row 0 of a plain 224-row causal prefill of the same data,
# without any padding.  That is the int8 contract's, not the padding's, and outside these bounds either way.
CONTRACT = [(33, 1), (95, 5), (193, 5), (224, 1), (100, 32), (100, 40), (224, 40), (224, 160)]


def contract_inputs(L, Nq, d, dist):
    h = 2
    Q, K, V = rr.inputs(Nq, 224, h * d, 1, dist, 9100 + L + 7 * Nq + d + (1 if dist == "uniform" else 0))
    return Q, K, V, h


@pytest.mark.parametrize("dist", rr.DISTS)
@pytest.mark.parametrize("d", [32, 64, 128])
def test_padded_contract_int8_against_float64(oracle_mod, d, dist):
    """rect_ref.fa_int8 on the padded operands, rows [s, s + Nq), within the project's 5e-3 of float64 attention of the
    Nq real rows over the L real keys."""
    worst = 0.0
    for L, Nq in CONTRACT:
        Q, K, V, h = contract_inputs(L, Nq, d, dist)
        Qp, Kp, Vp, s = padded_operands(Q, K, V, L)
        got = rr.fa_int8(oracle_mod, Qp, Kp, Vp, h * d, h, causal=True)[0][:, s:s + Nq]
        ref = rr.attention_f64(Q, K[:, :L], V[:, :L], h * d, h, causal=True)
        err = float(np.abs(got - ref).max())
        worst = max(worst, err)
        print(f"int8 d{d} {dist} L{L} Nq{Nq} s{s}: max|padded contract - float64| = {err:.2e} (bound 5e-3)")
        assert np.isfinite(got).all() and err <= 5e-3, (L, Nq, err)
    print(f"int8 d{d} {dist}: worst {worst:.2e}")


@pytest.mark.parametrize("dist", rr.DISTS)
@pytest.mark.parametrize("d", [64, 128])
def test_padded_contract_fp16_against_float64(d, dist):
    """rect_ref.fa_fp16_lazy on the padded operands, rows [s, s + Nq), within max(1e-3, 1e-3 |ref|) of float64."""
    for L, Nq in CONTRACT:
        Q, K, V, h = contract_inputs(L, Nq, d, dist)
        Qp, Kp, Vp, s = padded_operands(Q, K, V, L)
        got = rr.fa_fp16_lazy(None, Qp, Kp, Vp, h * d, h, causal=True)[:, s:s + Nq]
        ref = rr.attention_f64(Q, K[:, :L], V[:, :L], h * d, h, causal=True)
        err = np.abs(got - ref)
        print(f"fp16 d{d} {dist} L{L} Nq{Nq} s{s}: max|padded contract - float64| = {float(err.max()):.2e}")
        assert np.isfinite(got).all() and (err <= np.maximum(1e-3, 1e-3 * np.abs(ref))).all(), (L, Nq, float(err.max()))
