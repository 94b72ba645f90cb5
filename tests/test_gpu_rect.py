"""GPU tests (MI355X) of rectangular attention: qmha_solve_rect and its bindings.

References (tests/rect_ref.py: the square restatements of tests/causal_ref.py on Q padded into the last rows, held
to float64 rectangular attention by tests/test_rect_cpu.py) and bounds, the project's own:
  * fa_tc_int8_b: EVERY element within 2 u_r + 5e-5 of the restatement in the kernels' base-2 score arithmetic
    (u_r: the row's one-flip unit, tests/causal_ref.py).
  * fa_tc_v1a: within fp16_lazy_tol(Nk) of its own contract (fa_fp16_lazy) and within max(1e-3, 1e-3 |ref|) of
    float64 rectangular attention.
  * shifted superdiagonal (every row's strongest key is its first masked one): int8 2 one-flip units, fp16
    2^-10 max|V|; tests/test_rect_cpu.py shows two wrong masks hundreds of times outside these.
  * HARD SHAPES (rect_ref.HARD_SHAPES: causal_ref's hard cases cut to rectangles): inputs that take the rectangular
    kernels' own int8 re-anchor, fp16 rebase and guards, with and without the mask, at the same two bounds;
    tests/test_rect_hard_cpu.py shows a re-anchor or rebase without its rescale hundreds of times outside them.
    Batch-chunked calls (qmha_set_overlap_chunks) with Nq != Nk are held bit for bit to the unchunked call.
Every call writes O into a buffer with a sentinel-filled guard behind it, which must come back untouched.
The observed maxima are printed in pytest's terminal summary (tests/parity_log.py).
"""
import ctypes
import functools

import numpy as np
import pytest

from tests import causal_ref as cr
from tests import parity_log
from tests import rect_ref as rr
from tests.gpu_support import (CAUSAL, F16, GUARD, INT8, assert_f16, assert_int8, c_solve, compiled_module, dev,  # noqa: F401
                               overlap_chunks, to_dev)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
TAG = "+r"  # this file's mark on its parity_log records
_ids = lambda v: rr.case_id(v) if isinstance(v, tuple) and len(v) == 6 else str(v)  # noqa: E731


def solve_rect(variant, t, d_model, h, flags, **kw):
    """qmha_solve_rect on device tensors t = [Q [B, Nq, d_model], K, V [B, Nk, d_model]]; O (numpy) through the guard."""
    assert t[0].shape[-1] == d_model
    return c_solve("rect", variant, t, h, flags, **kw)


def solve_opts(variant, t, d_model, h, flags):
    assert t[0].shape[-1] == d_model
    return c_solve("opts", variant, t, h, flags)


# ---- parity ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def int8_reference(case, dist):
    """(Q, K, V, O_ref in the kernels' base-2 arithmetic, per-element one-flip unit), computed once and shared."""
    from oracle import oracle
    Nq, Nk, d_model, h, B, causal = case
    Q, K, V = rr.inputs(Nq, Nk, d_model, B, dist, rr.seed_of(case, dist))
    ref, unit = rr.fa_int8(oracle, Q, K, V, d_model, h, causal=causal, base2=True)
    return Q, K, V, ref, cr.per_element(unit, d_model // h)


@functools.lru_cache(maxsize=None)
def f16_reference(case, dist):
    Nq, Nk, d_model, h, B, causal = case
    Q, K, V = rr.inputs(Nq, Nk, d_model, B, dist, rr.seed_of(case, dist))
    return (Q, K, V, rr.fa_fp16_lazy(None, Q, K, V, d_model, h, causal=causal),
            rr.attention_f64(Q, K, V, d_model, h, causal))


@pytest.mark.parametrize("dist", rr.DISTS)
@pytest.mark.parametrize("case", rr.INT8_CASES, ids=_ids)
def test_int8_rect_vs_base2_restatement(dev, case, dist):
    Nq, Nk, d_model, h, B, causal = case
    Q, K, V, ref, unit = int8_reference(case, dist)
    got = solve_rect(INT8, to_dev(dev, Q, K, V), d_model, h, CAUSAL if causal else 0)
    assert_int8(f"{rr.case_id(case)} {dist}", got, ref, unit, TAG)


@pytest.mark.parametrize("dist", rr.DISTS)
@pytest.mark.parametrize("case", rr.F16_CASES, ids=_ids)
def test_fp16_rect_vs_lazy_contract_and_float64(dev, case, dist):
    Nq, Nk, d_model, h, B, causal = case
    Q, K, V, contract, exact = f16_reference(case, dist)
    got = solve_rect(F16, to_dev(dev, Q, K, V), d_model, h, CAUSAL if causal else 0)
    assert_f16(f"{rr.case_id(case)} {dist}", got, contract, cr.fp16_lazy_tol(Nk), TAG, exact)


# ---- the mask: every row's strongest key is its first masked one ----------------------------------------------
@pytest.mark.parametrize("shape", rr.SUPERDIAG, ids=str)
def test_int8_shifted_superdiagonal(dev, shape):
    from oracle import oracle
    Nq, Nk, d_model, h, B = shape
    Q, K, V = rr.superdiag_inputs(Nq, Nk, d_model, B)
    ref, unit = rr.fa_int8(oracle, Q, K, V, d_model, h, causal=True, base2=True)
    got = solve_rect(INT8, to_dev(dev, Q, K, V), d_model, h, CAUSAL)
    assert_int8(f"superdiag {shape}", got, ref, cr.per_element(unit, d_model // h), TAG)


@pytest.mark.parametrize("shape", [s for s in rr.SUPERDIAG if s[2] // s[3] in (64, 128)], ids=str)
def test_fp16_shifted_superdiagonal(dev, shape):
    """Against the contract only: with p up to 2^12 rounded to half the contract itself is ~1e-2 from float64 on
    these inputs (a property of fp16 p)."""
    Nq, Nk, d_model, h, B = shape
    Q, K, V = rr.superdiag_inputs(Nq, Nk, d_model, B)
    ref = rr.fa_fp16_lazy(None, Q, K, V, d_model, h, causal=True)
    got = solve_rect(F16, to_dev(dev, Q, K, V), d_model, h, CAUSAL)
    assert_f16(f"superdiag {shape}", got, ref, 2.0 ** -10 * float(np.abs(V).max()), TAG)


# ---- chunked prefill -------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant,d", [(INT8, 32), (INT8, 64), (F16, 64)])
def test_chunked_prefill_reproduces_full_prefill(dev, variant, d):
    """N = 256 in chunks of 64 rows: chunk c is qmha_solve_rect(Q[64c : 64c + 64], K[: 64(c + 1)], V[: 64(c + 1)], causal).
    The concatenation is held to the square causal reference at N = 256 and to the GPU's own
    qmha_solve_opts(CAUSAL) result, both at the variant's bound."""
    from oracle import oracle
    N, C, h, B = 256, 64, 2, 2
    d_model = h * d
    Q, K, V = cr.inputs(N, d_model, B, "normal", 500 + d)
    t = to_dev(dev, Q, K, V)
    parts = []
    for c in range(N // C):
        n = C * (c + 1)
        tc = [t[0][:, n - C:n].contiguous(), t[1][:, :n].contiguous(), t[2][:, :n].contiguous()]
        parts.append(solve_rect(variant, tc, d_model, h, CAUSAL))
    got = np.concatenate(parts, axis=1)
    square = solve_opts(variant, t, d_model, h, CAUSAL)
    same = np.array_equal(got, square)
    print(f"{variant} d{d}: chunked prefill {'is' if same else 'is NOT'} bit-identical to the square causal call"
          f" (max difference {np.abs(got - square).max():.3e})")
    if variant == INT8:
        ref, unit, _ = cr.fa_int8(oracle, Q, K, V, d_model, h, causal=True, base2=True)
        pe = cr.per_element(unit, d)
        assert_int8(f"chunked prefill d{d}", got, ref, pe, TAG)
        assert_int8(f"chunked prefill d{d} (vs the square GPU call)", got, square.astype(np.float64), pe, TAG)
    else:
        ref = cr.fa_fp16_lazy(None, Q, K, V, d_model, h, causal=True)[0]
        assert_f16(f"chunked prefill d{d}", got, ref, cr.fp16_lazy_tol(N), TAG, cr.attention_f64(Q, K, V, d_model, h, causal=True))
        assert_f16(f"chunked prefill d{d} (vs the square GPU call)", got, square, cr.fp16_lazy_tol(N), TAG)


# ---- routing -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant,flags", [("fa", 0), (F16, 0), (INT8, 0), ("unfused", 0), ("fa_mfma", 0),
                                           ("fa_tc_int8_pt", 0), (INT8, CAUSAL), (F16, CAUSAL)])
def test_square_calls_are_qmha_solve_opts(dev, variant, flags):
    N, d_model, h = 96, 128, 2
    t = to_dev(dev, *cr.inputs(N, d_model, 2, "normal", 510))
    assert np.array_equal(solve_rect(variant, t, d_model, h, flags), solve_opts(variant, t, d_model, h, flags))


@pytest.mark.parametrize("variant", [INT8, F16])
@pytest.mark.parametrize("case", [rr.CASES[2], rr.CASES[5]], ids=_ids)
def test_repeatable_and_batch_independent(dev, variant, case):
    """The same call twice is bit-identical; each sequence of a B = 2 call equals its own B = 1 call."""
    Nq, Nk, d_model, h, B, causal = case
    flags = CAUSAL if causal else 0
    t = to_dev(dev, *rr.inputs(Nq, Nk, d_model, B, "normal", 520))
    a = solve_rect(variant, t, d_model, h, flags)
    assert np.array_equal(a, solve_rect(variant, t, d_model, h, flags))
    for b in range(B):
        one = solve_rect(variant, [x[b:b + 1].contiguous() for x in t], d_model, h, flags)
        assert np.array_equal(one[0], a[b])


@pytest.mark.parametrize("variant", [INT8, F16])
def test_caller_workspace_on_a_side_stream_and_profile_marks(dev, variant):
    """Caller-owned scratch of exactly qmha_workspace_size(B, Nk, ...) bytes on a non-default stream equals the
    leased-slot result; one byte less is refused; with profiling on, every call is recorded with a main-kernel and
    a pre-pass time."""
    from quantizedmha_amd import _lib
    lib = _lib.load()
    Nq, Nk, d_model, h, B, _ = rr.CASES[2]
    t = to_dev(dev, *rr.inputs(Nq, Nk, d_model, B, "uniform", 530))
    want = solve_rect(variant, t, d_model, h, CAUSAL)
    need = lib.qmha_workspace_size(B, Nk, d_model, h, _lib.VARIANTS[variant])
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    assert np.array_equal(solve_rect(variant, t, d_model, h, CAUSAL, ws=ws, stream=s.cuda_stream), want)
    solve_rect(variant, t, d_model, h, CAUSAL, ws=ws, ws_bytes=need - 1, stream=s.cuda_stream, expect=1)
    lib.qmha_profile_collect(None, None, None)
    lib.qmha_profile_enable(1)
    try:
        for _ in range(3):
            assert np.array_equal(solve_rect(variant, t, d_model, h, CAUSAL), want)
        main_ms, pre_ms, calls = ctypes.c_double(), ctypes.c_double(), ctypes.c_longlong()
        assert lib.qmha_profile_collect(ctypes.byref(main_ms), ctypes.byref(calls), ctypes.byref(pre_ms)) == 0
    finally:
        lib.qmha_profile_enable(0)
    assert calls.value == 3 and main_ms.value > 0.0 and pre_ms.value > 0.0, (calls.value, main_ms.value, pre_ms.value)


@pytest.mark.parametrize("variant,d_model,h", [("fa", 128, 2), ("unfused", 128, 2), ("fa_mfma", 128, 2),
                                               ("fa_tc_int8_pt", 128, 2), (INT8, 192, 2), (F16, 64, 2)])
@pytest.mark.parametrize("flags", [0, CAUSAL])
def test_unsupported_rect_touches_nothing(dev, variant, d_model, h, flags):
    from quantizedmha_amd import _lib
    Q, K, V = rr.inputs(64, 128, d_model, 1, "normal", 540)
    got = solve_rect(variant, to_dev(dev, Q, K, V), d_model, h, flags, expect=4)
    assert (got == GUARD).all()
    msg = _lib.load().qmha_last_error().decode()
    assert variant in msg and f"d = {d_model // h}" in msg


# ---- bindings ------------------------------------------------------------------------------------------
def test_bindings_route_to_qmha_solve_rect(dev):
    """torch_ext.flash_solve_rect (the Python mirror, with out=, and the compiled module) gives the C-ABI's result
    bit for bit; mismatched K / V and batch counts raise; flash_solve still wants one shape."""
    from quantizedmha_amd import torch_ext
    Nq, Nk, d_model, h, B = 96, 160, 128, 2, 2
    t = to_dev(dev, *rr.inputs(Nq, Nk, d_model, B, "normal", 550))
    compiled = compiled_module()
    for variant in (INT8, F16):
        for causal in (False, True):
            want = solve_rect(variant, t, d_model, h, CAUSAL if causal else 0)
            out = torch.empty_like(t[0])
            got = torch_ext.flash_solve_rect(t[0], t[1], t[2], d_model, h, variant, out=out, causal=causal)
            torch.cuda.synchronize()
            assert got is out and np.array_equal(out.cpu().numpy(), want)
            got = compiled.flash_solve_rect(t[0], t[1], t[2], d_model, h, variant, causal=causal)
            torch.cuda.synchronize()
            assert got.shape == t[0].shape and np.array_equal(got.cpu().numpy(), want)
    one = torch_ext.flash_solve_rect(t[0][0], t[1][0], t[2][0], d_model, h)  # [Nq, d_model] against [Nk, d_model]
    torch.cuda.synchronize()
    assert np.array_equal(one.cpu().numpy(), solve_rect(INT8, [x[:1].contiguous() for x in t], d_model, h, 0)[0])
    for mod in (torch_ext, compiled):
        with pytest.raises(RuntimeError, match="K and V must have the same shape"):
            mod.flash_solve_rect(t[0], t[1], t[2][:, :128].contiguous(), d_model, h)
        with pytest.raises(RuntimeError, match="same batch count"):
            mod.flash_solve_rect(t[0][:1].contiguous(), t[1], t[2], d_model, h)
        with pytest.raises(RuntimeError, match="same shape"):
            mod.flash_solve(t[0], t[1], t[2], d_model, h)
    with pytest.raises(RuntimeError, match="not supported"):
        torch_ext.flash_solve_rect(t[0], t[1], t[2], d_model, h, "fa")
    with pytest.raises(RuntimeError, match="Nk >= Nq"):
        torch_ext.flash_solve_rect(t[1], t[0], t[0], d_model, h, causal=True)


# ---- hard numerics: the rectangular kernels' own re-anchor (int8), rebase (fp16) and guards ---------------------
# rect_ref.HARD_SHAPES; tests/test_rect_hard_cpu.py shows which branch each shape takes and that a
# re-anchor / rebase without its rescale of l or of O is hundreds of times outside the bounds used here.
@functools.lru_cache(maxsize=None)
def hard_int8_reference(shape, d):
    """(Q, K, V, O_ref in the kernels' base-2 arithmetic, per-element one-flip unit), computed once and shared."""
    from oracle import oracle
    c = cr.HARD[shape.name]
    Q, K, V = rr.hard_inputs(shape.name, d, shape.Nq, shape.Nk)
    ref, unit = rr.fa_int8(oracle, Q, K, V, c.h * d, c.h, causal=shape.causal, base2=True)
    return Q, K, V, ref, cr.per_element(unit, d)


@functools.lru_cache(maxsize=None)
def hard_f16_reference(shape, d):
    c = cr.HARD[shape.name]
    Q, K, V = rr.hard_inputs(shape.name, d, shape.Nq, shape.Nk)
    return Q, K, V, rr.fa_fp16_lazy(None, Q, K, V, c.h * d, c.h, causal=shape.causal)


def hard_flip_tol(V):
    """2^-10 max|V|: one flipped half(p) of a dominant key, the fp16 bound of the hard cases."""
    return 2.0 ** -10 * float(np.abs(V).max())


@pytest.mark.parametrize("shape,d", rr.HARD_INT8, ids=rr.hard_id)
def test_int8_hard_shapes_vs_base2_restatement(dev, shape, d):
    """Every element finite and within 2 u_r + 5e-5 of rect_ref.fa_int8(base2=True); `underflow` and V = 0 give exactly
    0 from the reference and from the GPU; `nan_int8` (a NaN in the Q slice, two each in K and V) gives the
    restatement's finite output."""
    c = cr.HARD[shape.name]
    flags = CAUSAL if shape.causal else 0
    Q, K, V, ref, unit = hard_int8_reference(shape, d)
    got = solve_rect(INT8, to_dev(dev, Q, K, V), c.h * d, c.h, flags)
    assert_int8(f"hard {rr.hard_id(shape)} d{d}", got, ref, unit, TAG)
    if shape.name == "underflow":
        assert not ref.any() and not got.any()
        assert not solve_rect(INT8, to_dev(dev, *rr.zero_v_hard_inputs(d, shape.Nq, shape.Nk)), c.h * d, c.h, flags).any()


@pytest.mark.parametrize("shape,d", rr.HARD_F16, ids=rr.hard_id)
def test_fp16_hard_shapes_vs_lazy_contract(dev, shape, d):
    """Finite and within 2^-10 max|V| of rect_ref.fa_fp16_lazy; `underflow` and V = 0 give exactly 0.  The distance to
    float64 is recorded only, for the reason given at tests/test_gpu_causal.py test_fp16_hard_cases_vs_lazy_contract."""
    c = cr.HARD[shape.name]
    flags = CAUSAL if shape.causal else 0
    Q, K, V, ref = hard_f16_reference(shape, d)
    got = solve_rect(F16, to_dev(dev, Q, K, V), c.h * d, c.h, flags)
    label = f"hard {rr.hard_id(shape)} d{d}"
    assert_f16(label, got, ref, hard_flip_tol(V), TAG)
    if shape.name == "underflow":  # float64 has no m0 = 0 guard
        assert not ref.any() and not got.any()
        assert not solve_rect(F16, to_dev(dev, *rr.zero_v_hard_inputs(d, shape.Nq, shape.Nk)), c.h * d, c.h, flags).any()
    else:
        far = float(np.abs(got - rr.attention_f64(Q, K, V, c.h * d, c.h, shape.causal)).max())
        parity_log.record(f"{label} (vs float64, recorded only)", F16 + TAG, far, 0.0, float("inf"))
        print(f"{label}: max|gpu - float64| = {far:.2e} (recorded only)")


@pytest.mark.parametrize("variant,shape,d", [(INT8,) + sd for sd in rr.HARD_INT8 if sd[0].causal]
                         + [(F16,) + sd for sd in rr.HARD_F16 if sd[0].causal], ids=rr.hard_id)
def test_hard_last_chunk_equals_the_square_causal_call(dev, variant, shape, d):
    """A causal hard shape is the last chunk of the square hard problem at N = Nk: the rectangular call is held to the
    last Nq rows of the GPU's own qmha_solve_opts(CAUSAL) at the variant's bound (whether they are bit-identical is
    printed)."""
    c = cr.HARD[shape.name]
    sq = c.build(d, c.h, shape.Nk, c.B)
    Q, K, V = rr.hard_inputs(shape.name, d, shape.Nq, shape.Nk)
    assert np.array_equal(Q, sq[0][:, -shape.Nq:], equal_nan=True) and np.array_equal(K, sq[1], equal_nan=True)
    got = solve_rect(variant, to_dev(dev, Q, K, V), c.h * d, c.h, CAUSAL)
    square = solve_opts(variant, to_dev(dev, *sq), c.h * d, c.h, CAUSAL)[:, -shape.Nq:]
    label = f"hard {rr.hard_id(shape)} d{d} (vs the square GPU call)"
    print(f"{variant} {label}: {'is' if np.array_equal(got, square) else 'is NOT'} bit-identical"
          f" (max difference {np.abs(got - square).max():.3e})")
    assert np.isfinite(square).all()
    if variant == INT8:
        assert_int8(label, got, square.astype(np.float64), hard_int8_reference(shape, d)[4], TAG)
    else:
        assert_f16(label, got, square, hard_flip_tol(V), TAG)


@pytest.mark.parametrize("variant,d", [(INT8, 32), (INT8, 64), (INT8, 128), (F16, 64), (F16, 128)])
def test_rows_before_the_spike_tile_are_bit_identical(dev, variant, d):
    """`spike_tile` (160, 256) causal: the query rows are rows 96..255 of the square problem and keys 160..191 one key
    tile, so rows 0..63 (waves 0 and 1 of the first workgroup, which skip that tile's body) equal the run without
    the spike bit for bit; every row from 64 on changes."""
    c = cr.HARD["spike_tile"]
    spike = solve_rect(variant, to_dev(dev, *rr.hard_inputs("spike_tile", d, 160, 256)), c.h * d, c.h, CAUSAL)
    plain = solve_rect(variant, to_dev(dev, *rr.hard_inputs("spike_tile", d, 160, 256, spike=False)), c.h * d, c.h, CAUSAL)
    assert np.array_equal(spike[:, :64], plain[:, :64])
    assert (spike[:, 64:] != plain[:, 64:]).any(axis=-1).all()


@pytest.mark.parametrize("variant,shape,d", [(INT8,) + sd for sd in rr.HARD_INT8] + [(F16,) + sd for sd in rr.HARD_F16],
                         ids=rr.hard_id)
def test_hard_shapes_repeat_and_split_by_batch(dev, variant, shape, d):
    """A hard shape run twice is bit-identical (nqb >= 2: the second pass of an int8 q-block pair restarts from
    anchor = 0, m = 0, l = 0 after the first re-anchored); each sequence of the B = 2 case equals its own B = 1 call."""
    c = cr.HARD[shape.name]
    flags = CAUSAL if shape.causal else 0
    t = to_dev(dev, *rr.hard_inputs(shape.name, d, shape.Nq, shape.Nk))
    a = solve_rect(variant, t, c.h * d, c.h, flags)
    assert np.isfinite(a).all() and np.array_equal(a, solve_rect(variant, t, c.h * d, c.h, flags))
    for b in range(c.B if c.B > 1 else 0):
        one = solve_rect(variant, [x[b:b + 1].contiguous() for x in t], c.h * d, c.h, flags)
        assert np.array_equal(one[0], a[b])


@pytest.mark.parametrize("variant", [INT8, F16])
@pytest.mark.parametrize("Nq,Nk,causal", [(96, 160, True), (160, 96, False)])
def test_overlap_chunks_with_rectangular_slabs_are_bit_identical(dev, variant, Nq, Nk, causal):
    """qmha_set_overlap_chunks(2 and 3) with B = 3 and Nq != Nk: every chunk boundary has b0 > 0, chunk c reads Q and
    writes O at b0 Nq d_model and reads K, V and its workspace slice at b0 Nk ..., and the two slabs differ in both
    directions over the two shapes.  Each run equals the unchunked call bit for bit, with the guard behind O intact."""
    B, d_model, h = 3, 128, 2
    flags = CAUSAL if causal else 0
    t = to_dev(dev, *rr.inputs(Nq, Nk, d_model, B, "normal", 560 + Nq))
    with overlap_chunks(1) as lib:
        want = solve_rect(variant, t, d_model, h, flags)
        assert len({want[b].tobytes() for b in range(B)}) == B  # three different sequences: a mixed-up slab shows
        for chunks in (2, 3):
            lib.qmha_set_overlap_chunks(chunks)
            for _ in range(2):
                assert np.array_equal(solve_rect(variant, t, d_model, h, flags), want), (variant, chunks)
