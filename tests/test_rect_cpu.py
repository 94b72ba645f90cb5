"""CPU tests of rectangular attention: the references of tests/rect_ref.py, the C-ABI checks
of qmha_solve_rect (they fail before any launch, so no device is needed) and the shipped kernel instances.

tests/rect_ref.py builds every rectangular reference from the square restatements of tests/causal_ref.py
(a rectangular result is a slice of a square one).  Here that construction is held to
  * causal_ref itself at Nq == Nk (exactly), and
  * a float64 rectangular attention written below, mask j > r + Nk - Nq, within the quantisation budgets
    of the two paths (int8 5e-3, fp16 1e-3; worst observed 3.5e-3 and 1.2e-4),
and the shifted-superdiagonal inputs are shown to put two wrong masks far outside the GPU tests' bounds.
"""
import ctypes
import functools
import os
import re
import subprocess

import numpy as np
import pytest

from tests import causal_ref as cr
from tests import rect_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAUSAL = 1
ALL_CASES = [(c, dist) for c in rr.INT8_CASES for dist in rr.DISTS]
ALL_F16_CASES = [(c, dist) for c in rr.F16_CASES for dist in rr.DISTS]
_ids = lambda v: rr.case_id(v) if isinstance(v, tuple) else str(v)  # noqa: E731


@pytest.fixture(scope="module")
def built():
    from tools.build import build
    build(verbose=False)
    return True


def rect_attention_f64(Q, K, V, d_model, h, causal):
    """float64 softmax(Q K^T / sqrt(d)) V, head by head; causal masks j > r + Nk - Nq."""
    Q, K, V = (np.asarray(x, np.float64) for x in (Q, K, V))
    B, Nq, _ = Q.shape
    Nk, d = K.shape[1], d_model // h
    out = np.zeros_like(Q)
    masked = np.arange(Nk)[None, :] > np.arange(Nq)[:, None] + Nk - Nq
    for b in range(B):
        for k in range(h):
            c = slice(k * d, (k + 1) * d)
            s = Q[b, :, c] @ K[b, :, c].T / np.sqrt(d)
            if causal:
                s[masked] = -np.inf
            p = np.exp(s - s.max(axis=1, keepdims=True))
            out[b, :, c] = (p / p.sum(axis=1, keepdims=True)) @ V[b, :, c]
    return out


# ---- the construction ---------------------------------------------------------------------------------
@pytest.mark.parametrize("causal", [True, False])
def test_square_construction_is_causal_ref(oracle_mod, causal):
    N, d_model, h, B = 96, 128, 2, 2
    Q, K, V = cr.inputs(N, d_model, B, "normal", 401)
    for base2 in (False, True):
        want, unit, _ = cr.fa_int8(oracle_mod, Q, K, V, d_model, h, causal=causal, base2=base2)
        got, got_unit = rr.fa_int8(oracle_mod, Q, K, V, d_model, h, causal=causal, base2=base2)
        assert np.array_equal(got, want) and np.array_equal(got_unit, unit)
    want = cr.fa_fp16_lazy(None, Q, K, V, d_model, h, causal=causal)[0]
    assert np.array_equal(rr.fa_fp16_lazy(None, Q, K, V, d_model, h, causal=causal), want)
    assert np.array_equal(rr.attention_f64(Q, K, V, d_model, h, causal), cr.attention_f64(Q, K, V, d_model, h, causal))


@pytest.mark.parametrize("case,dist", ALL_CASES, ids=_ids)
def test_int8_restatements_within_quantisation_budget(oracle_mod, case, dist):
    """Both forms of the int8 restatement (nats: the C oracle's; base 2: the kernels') within 5e-3 of float64, and
    within a few one-flip units of each other (recorded)."""
    Nq, Nk, d_model, h, B, causal = case
    Q, K, V = rr.inputs(Nq, Nk, d_model, B, dist, rr.seed_of(case, dist))
    exact = rect_attention_f64(Q, K, V, d_model, h, causal)
    assert np.allclose(exact, rr.attention_f64(Q, K, V, d_model, h, causal), rtol=0, atol=1e-12)
    nats, unit = rr.fa_int8(oracle_mod, Q, K, V, d_model, h, causal=causal)
    two, _ = rr.fa_int8(oracle_mod, Q, K, V, d_model, h, causal=causal, base2=True)
    assert nats.shape == Q.shape and unit.shape == (B, Nq, h)
    for name, got in (("nats", nats), ("base2", two)):
        err = float(np.abs(got - exact).max())
        print(f"{rr.case_id(case)} {dist} {name}: max|restatement - float64| = {err:.2e} (budget 5e-3)")
        assert np.isfinite(got).all() and err <= 5e-3, (name, err)
    apart = cr.flip_units(np.abs(two.astype(np.float64) - nats), cr.per_element(unit, d_model // h))
    print(f"{rr.case_id(case)} {dist}: base 2 and nats forms {apart:.2f} one-flip units apart")


@pytest.mark.parametrize("case,dist", ALL_F16_CASES, ids=_ids)
def test_fp16_restatement_within_quantisation_budget(case, dist):
    Nq, Nk, d_model, h, B, causal = case
    Q, K, V = rr.inputs(Nq, Nk, d_model, B, dist, rr.seed_of(case, dist))
    got = rr.fa_fp16_lazy(None, Q, K, V, d_model, h, causal=causal)
    err = float(np.abs(got - rect_attention_f64(Q, K, V, d_model, h, causal)).max())
    print(f"{rr.case_id(case)} {dist}: max|lazy contract - float64| = {err:.2e} (budget 1e-3)")
    assert got.shape == Q.shape and np.isfinite(got).all() and err <= 1e-3, err


def test_causal_rows_see_their_prefix_only(oracle_mod):
    """Row r of a causal call depends on keys j <= r + Nk - Nq only: negating K and V from key j0 on (a sign flip
    keeps every group's absmax) leaves the rows whose group lies before j0's bit-identical and changes every row
    from j0 - (Nk - Nq) on."""
    Nq, Nk, d_model, h = 64, 160, 128, 2
    Q, K, V = rr.inputs(Nq, Nk, d_model, 1, "normal", 402)
    j0 = 96 + 32 + 13  # in the second query group's diagonal tile
    K2, V2 = K.copy(), V.copy()
    K2[:, j0:] *= -1
    V2[:, j0:] *= -1
    r0 = j0 - (Nk - Nq)
    for base, neg in ((rr.fa_int8(oracle_mod, Q, K, V, d_model, h, causal=True)[0],
                       rr.fa_int8(oracle_mod, Q, K2, V2, d_model, h, causal=True)[0]),
                      (rr.fa_fp16_lazy(None, Q, K, V, d_model, h, causal=True),
                       rr.fa_fp16_lazy(None, Q, K2, V2, d_model, h, causal=True))):
        assert np.array_equal(neg[:, :32], base[:, :32])
        assert (neg[:, r0:] != base[:, r0:]).any(axis=-1).all()


# ---- the tests can fail: two wrong masks on the shifted superdiagonal ----------------------------------------
MUTANTS = ["mask_after_max", "leak_next"]
# a quarter of the smallest distance measured over SUPERDIAG with these inputs: int8 335..670 and 2030..6392 one-flip
# units (GPU bound 2), fp16 784..989 and 1258..1389 times the GPU bound 2^-10 max|V|
INT8_MUTANT_UNITS = {"mask_after_max": 335 / 4, "leak_next": 2030 / 4}
F16_MUTANT_BOUNDS = {"mask_after_max": 784 / 4, "leak_next": 1258 / 4}


@functools.lru_cache(maxsize=None)
def superdiag(shape):
    Nq, Nk, d_model, h, B = shape
    return rr.superdiag_inputs(Nq, Nk, d_model, B)


@pytest.mark.parametrize("mutant", MUTANTS)
@pytest.mark.parametrize("shape", rr.SUPERDIAG, ids=str)
def test_int8_mask_mutants_are_far_outside_the_gpu_bound(oracle_mod, shape, mutant):
    """K[Nk - Nq + 1 + r] = 32 Q[r]: the first masked key of every row is its strongest.  A mask applied after the
    row max, or one key late, lands hundreds of one-flip units from the correct result (GPU bound: 2)."""
    Nq, Nk, d_model, h, B = shape
    Q, K, V = superdiag(shape)
    ref, unit = rr.fa_int8(oracle_mod, Q, K, V, d_model, h, causal=True, base2=True)
    bad, _ = rr.fa_int8(oracle_mod, Q, K, V, d_model, h, causal=True, base2=True, _mutant=mutant)
    units = cr.flip_units(np.abs(bad.astype(np.float64) - ref), cr.per_element(unit, d_model // h))
    print(f"superdiag {shape} {mutant}: {units:.0f} one-flip units from the correct mask")
    assert units >= INT8_MUTANT_UNITS[mutant], units


@pytest.mark.parametrize("mutant", MUTANTS)
@pytest.mark.parametrize("shape", [s for s in rr.SUPERDIAG if s[2] // s[3] in (64, 128)], ids=str)
def test_fp16_mask_mutants_are_far_outside_the_gpu_bound(shape, mutant):
    Nq, Nk, d_model, h, B = shape
    Q, K, V = superdiag(shape)
    ref = rr.fa_fp16_lazy(None, Q, K, V, d_model, h, causal=True)
    bad = rr.fa_fp16_lazy(None, Q, K, V, d_model, h, causal=True, _mutant=mutant)
    tol = 2.0 ** -10 * float(np.abs(V).max())
    err = float(np.abs(bad - ref).max())
    print(f"superdiag {shape} {mutant}: {err / tol:.0f} x the GPU bound")
    assert err >= F16_MUTANT_BOUNDS[mutant] * tol, (err, tol)


# ---- C-ABI argument checks: they fail before any launch ------------------------------------------------------
def rect_status(lib, B, Nq, Nk, d_model, h, vid, flags, ws=None, ws_bytes=0, Q=0x1000):
    dummy = ctypes.c_void_p(0x1000)  # never dereferenced: checks run first
    st = lib.qmha_solve_rect(ctypes.c_void_p(Q) if Q else None, dummy, dummy, dummy, B, Nq, Nk, d_model, h, vid, flags,
                             ws, ws_bytes, None)
    return st, lib.qmha_last_error().decode()


@pytest.mark.parametrize("args,status,cause", [
    ((1, 100, 128, 128, 2, 2, 0), 1, "Nq must be a multiple of 32"),
    ((1, 128, 100, 128, 2, 2, 0), 1, "Nk must be a multiple of 32"),
    ((1, 0, 128, 128, 2, 2, 0), 1, "positive"),
    ((1, 128, 0, 128, 2, 2, 0), 1, "positive"),
    ((1, 160, 128, 128, 2, 2, CAUSAL), 1, "Nk >= Nq"),
    ((1, 160, 128, 128, 2, 1, CAUSAL), 1, "Nk >= Nq"),
    ((1, 64, 128, 128, 2, 2, 2), 1, "flag"),
    ((1, 64, 128, 128, 2, 2, 0x80000001), 1, "flag"),
    ((1, 64, 128, 128, 3, 2, 0), 1, "divisible"),
    ((1, 64, 128, 128, 2, 7, 0), 1, "unknown variant"),
    ((1, 64, 128, 1024, 2, 2, 0), 4, "above 256"),
])
def test_rect_invalid_arguments_rejected_before_launch(built, args, status, cause):
    from quantizedmha_amd import _lib
    st, msg = rect_status(_lib.load(), *args)
    assert st == status and cause in msg, (st, msg)


def test_rect_null_pointer_is_invalid(built):
    from quantizedmha_amd import _lib
    st, msg = rect_status(_lib.load(), 1, 64, 128, 128, 2, 2, 0, Q=0)
    assert st == 1 and "null" in msg


@pytest.mark.parametrize("vid,name,d_model,h", [
    (0, "fa", 128, 2), (3, "unfused", 128, 2), (4, "fa_mfma", 128, 2), (5, "fa_tc_int8_pt", 128, 2),
    (2, "fa_tc_int8_b", 192, 2),  # d = 96
    (1, "fa_tc_v1a", 64, 2),      # d = 32: int8 only
])
@pytest.mark.parametrize("flags", [0, CAUSAL])
def test_rect_unsupported_combinations_are_nosys(built, vid, name, d_model, h, flags):
    from quantizedmha_amd import _lib
    lib = _lib.load()
    for ws in (None, ctypes.c_void_p(0x1000)):  # library-owned and caller-owned workspace forms
        st, msg = rect_status(lib, 1, 64, 128, d_model, h, vid, flags, ws, 1 << 30)
        assert st == 4, (st, msg)
        assert name in msg and f"d = {d_model // h}" in msg and "Nq != Nk" in msg, msg


@pytest.mark.parametrize("vid", [1, 2])
def test_rect_caller_workspace_one_byte_short_is_invalid(built, vid):
    """The scratch is that of the keys: qmha_workspace_size(B, Nk, ...), whatever Nq."""
    from quantizedmha_amd import _lib
    lib = _lib.load()
    B, Nq, Nk, d_model, h = 2, 32, 160, 128, 2
    need = lib.qmha_workspace_size(B, Nk, d_model, h, vid)
    assert need > lib.qmha_workspace_size(B, Nq, d_model, h, vid) > 0
    st, msg = rect_status(lib, B, Nq, Nk, d_model, h, vid, 0, ctypes.c_void_p(0x1000), need - 1)
    assert st == 1 and "workspace too small" in msg, (st, msg)


def test_rect_kernels_one_instance_per_head_size(built):
    """The causal switch is a runtime argument: one rectangular (Rect geometry) qmha_fa_int8_masked_kernel per d in
    {32, 64, 128} and one qmha_fa_f16_masked_kernel per d in {64, 128}; beside them exactly one square-causal
    (SquareCausal geometry) and one grouped-query (Grouped geometry) instance per head size, fifteen kernels in all."""
    path = os.path.join(ROOT, "quantizedmha_amd", "lib", "libqmha.so")
    syms = subprocess.run(["nm", path], capture_output=True, text=True, check=True).stdout
    stubs = sorted(re.findall(r"__device_stub__(qmha_fa_\w+?_masked_kernel)ILi(\d+)ENS_\d+([A-Za-z]+?)E(\w*)", syms))
    per_d = [("qmha_fa_f16_masked_kernel", 128), ("qmha_fa_f16_masked_kernel", 64), ("qmha_fa_int8_masked_kernel", 128),
             ("qmha_fa_int8_masked_kernel", 32), ("qmha_fa_int8_masked_kernel", 64)]
    for geo in ("Rect", "SquareCausal", "Grouped"):
        assert [(n, int(d)) for n, d, g, _ in stubs if g == geo] == per_d, (geo, stubs)
    assert len(stubs) == 15 and "_rect_kernel" not in syms and "_causal_kernel" not in syms, stubs
    # the rectangular instances take no template argument beyond (D, geometry): causal or not is decided at run time
    assert all(rest.startswith("EEv") for _, _, _, rest in stubs), stubs


def test_python_binding_has_flash_solve_rect():
    import inspect
    from quantizedmha_amd import torch_ext
    sig = inspect.signature(torch_ext.flash_solve_rect)
    assert list(sig.parameters) == ["Q", "K", "V", "d_model", "num_heads", "kernel", "out", "causal"]
    assert sig.parameters["causal"].default is False and sig.parameters["kernel"].default == "fa_tc_int8_b"
    torch = pytest.importorskip("torch")
    q = torch.zeros(64, 32)
    with pytest.raises(RuntimeError, match="Inputs must be CUDA tensors"):
        torch_ext.flash_solve_rect(q, torch.zeros(128, 32), torch.zeros(128, 32), 32, 1)
