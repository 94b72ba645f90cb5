"""GPU tests (MI355X) of causal attention: qmha_solve_opts(QMHA_FLAG_CAUSAL) and the bindings.

References and bounds:
  * fa_tc_int8_b against tests/causal_ref.py (the numpy restatement of the C oracle with the mask, itself held
    to the oracle by tests/test_causal_cpu.py): EVERY element within 2 u_r + 5e-5, u_r the row's one-flip
    unit (the most one Pi changing by 1 moves an element of the row).  The GPU's exp2 against the oracle's
    expf can move a p / sP across a .5 boundary, a rare ulp-level event; two in one row are not expected.  A
    leaked or dropped key moves a row by about |v| / l, some 30 units.
  * fa_tc_v1a against float64 masked attention within verify.cu's own max(1e-3, 1e-3 |ref|)
    (oracle.verify_results).
  * fa_tc_v1a against its own contract restated with the mask (causal_ref.fa_fp16_lazy, held to the C oracle's
    fa_fp16_lazy by the CPU tests): the committed cases within fp16_lazy_tol(N), the hard cases within
    2^-10 max|V| (one flipped half(p) of a dominant key, test_lazy_base_staircase's bound).
  * HARD CASES (causal_ref.HARD_CASES): inputs that take the int8 kernel's re-anchor branch and the fp16 kernel's
    rebase branch, on and off the diagonal tile, and that put the strongest key of every row just behind the
    mask.  int8 is compared with the restatement in the kernel's own base-2 score arithmetic (base2=True).
The observed maxima are printed in pytest's terminal summary (tests/parity_log.py): for int8 the worst
error in one-flip units with bound 2, for fp16 the worst absolute error with its bound.
"""
import ctypes
import functools
import json
import os
import subprocess

import numpy as np
import pytest

from tests import causal_ref as cr
from tests import parity_log
from tests.gpu_support import CAUSAL, F16, GUARD, INT8, assert_int8, c_solve, compiled_module, dev, to_dev  # noqa: F401
from tests.gpu_support import assert_f16 as assert_f16_contract  # this file's own assert_f16 is the float64 one

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAG = "+c"  # this file's mark on its parity_log records
INT8_CASES = cr.CASES + cr.CASES_INT8_D32
F16_CASES = [c for c in cr.CASES if c[1] // c[2] in (64, 128)] + cr.CASES_F16_EXTRA


def solve_opts(variant, t, d_model, h, flags, **kw):
    """qmha_solve_opts on device tensors t = [Q, K, V] ([B, N, d_model]); O (numpy) through the guard, after a sync."""
    assert t[0].shape[-1] == d_model
    return c_solve("opts", variant, t, h, flags, **kw)


def causal(variant, dev, Q, K, V, d_model, h):
    return solve_opts(variant, to_dev(dev, Q, K, V), d_model, h, CAUSAL)


@functools.lru_cache(maxsize=None)
def int8_reference(case):
    """(Q, K, V, O_ref, per-element one-flip unit) of a case, computed once and shared."""
    from oracle import oracle
    N, d_model, h, B, dist, seed = case
    Q, K, V = cr.inputs(N, d_model, B, dist, seed)
    ref, unit, _ = cr.fa_int8(oracle, Q, K, V, d_model, h, causal=True)
    return Q, K, V, ref, cr.per_element(unit, d_model // h)


# held to float64 alone, under the bare label: gpu_support.assert_f16 would need a flag that only this file sets
def assert_f16(label, got, ref):
    from oracle import oracle
    assert np.isfinite(got).all()
    err = float(np.abs(got - ref).max())
    parity_log.record(label, F16 + TAG, err, float((np.abs(got - ref) > 5e-5).mean()), 1e-3)
    print(f"{label}: max|gpu - float64| = {err:.3e} (bound max(1e-3, 1e-3 |ref|))")
    assert oracle.verify_results(got, ref.astype(np.float32), 1e-3, 1e-3) == -1, (label, err)


# ---- parity ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", INT8_CASES, ids=lambda c: f"N{c[0]}-d{c[1] // c[2]}-h{c[2]}-B{c[3]}-{c[4]}")
def test_int8_causal_vs_restatement(dev, case):
    N, d_model, h, B, dist, seed = case
    Q, K, V, ref, unit = int8_reference(case)
    assert_int8(f"N{N} d{d_model // h} B{B} {dist}", causal(INT8, dev, Q, K, V, d_model, h), ref, unit, TAG)


@pytest.mark.parametrize("case", F16_CASES, ids=lambda c: f"N{c[0]}-d{c[1] // c[2]}-h{c[2]}-B{c[3]}-{c[4]}")
def test_fp16_causal_vs_float64(dev, case):
    N, d_model, h, B, dist, seed = case
    Q, K, V = cr.inputs(N, d_model, B, dist, seed)
    ref = cr.attention_f64(Q, K, V, d_model, h, causal=True)
    assert_f16(f"N{N} d{d_model // h} B{B} {dist}", causal(F16, dev, Q, K, V, d_model, h), ref)


@functools.lru_cache(maxsize=None)
def f16_contract(case):
    N, d_model, h, B, dist, seed = case
    Q, K, V = cr.inputs(N, d_model, B, dist, seed)
    return Q, K, V, cr.fa_fp16_lazy(None, Q, K, V, d_model, h, causal=True)[0]


@pytest.mark.parametrize("case", F16_CASES, ids=lambda c: f"N{c[0]}-d{c[1] // c[2]}-h{c[2]}-B{c[3]}-{c[4]}")
def test_fp16_causal_vs_lazy_contract(dev, case):
    """Beside the float64 check: the kernel's own contract with the mask, at the non-causal kernel's bound against
    oracle.fa_fp16_lazy.  A late row of N >= 512 that drops or leaks one key moves by ~|v| / r ~ 5e-4: inside the
    float64 bound of 1e-3, ten times outside this one."""
    N, d_model, h, B, dist, seed = case
    Q, K, V, ref = f16_contract(case)
    got = causal(F16, dev, Q, K, V, d_model, h)
    assert_f16_contract(f"N{N} d{d_model // h} B{B} {dist}", got, ref, cr.fp16_lazy_tol(N), TAG)


# ---- hard numerics: re-anchor (int8), rebase (fp16), the strongest key behind the mask ---------------------
@functools.lru_cache(maxsize=None)
def hard_int8_reference(name, d, spike=True):
    """(Q, K, V, O_ref in the kernel's base-2 arithmetic, per-element one-flip unit), computed once and shared."""
    from oracle import oracle
    c = cr.HARD[name]
    Q, K, V = cr.hard_inputs(name, d) if spike else cr.hard_inputs(name, d, spike=False)
    ref, unit, _ = cr.fa_int8(oracle, Q, K, V, c.h * d, c.h, causal=True, base2=True)
    return Q, K, V, ref, cr.per_element(unit, d)


@functools.lru_cache(maxsize=None)
def hard_f16_reference(name, d):
    c = cr.HARD[name]
    Q, K, V = cr.hard_inputs(name, d)
    return Q, K, V, cr.fa_fp16_lazy(None, Q, K, V, c.h * d, c.h, causal=True)[0]


@pytest.mark.parametrize("name,d", cr.HARD_INT8, ids=str)
def test_int8_hard_cases_vs_base2_restatement(dev, name, d):
    """Every element within 2 u_r + 5e-5 of fa_int8(base2=True, causal=True) and finite; `underflow` and V = 0 give
    exactly 0; `nan_int8` (NaNs in Q, K and V) gives the restatement's finite output."""
    c = cr.HARD[name]
    Q, K, V, ref, unit = hard_int8_reference(name, d)
    got = causal(INT8, dev, Q, K, V, c.h * d, c.h)
    assert_int8(f"hard {name} d{d}", got, ref, unit, TAG)
    if name == "underflow":
        assert not ref.any() and not got.any()
        Q, K, V = cr.zero_v_inputs(d, c.h, c.N, c.B)
        assert not causal(INT8, dev, Q, K, V, c.h * d, c.h).any()


@pytest.mark.parametrize("name,d", cr.HARD_F16, ids=str)
def test_fp16_hard_cases_vs_lazy_contract(dev, name, d):
    """Within 2^-10 max|V| of fa_fp16_lazy(causal=True) and finite; `underflow` and V = 0 give exactly 0.  Not held
    to float64 at 1e-3: with p up to 2^12 rounded to half the CONTRACT is 5e-3..1e-2 from float64 on `staircase`
    and `superdiag` (a property of fp16 p); that distance is recorded."""
    c = cr.HARD[name]
    Q, K, V, ref = hard_f16_reference(name, d)
    got = causal(F16, dev, Q, K, V, c.h * d, c.h)
    assert_f16_contract(f"hard {name} d{d}", got, ref, 2.0 ** -10 * float(np.abs(V).max()), TAG)
    exact = cr.attention_f64(Q, K, V, c.h * d, c.h, causal=True)
    far = float(np.abs(got - exact).max()) if name != "underflow" else 0.0  # float64 has no m0 = 0 guard
    parity_log.record(f"hard {name} d{d} (vs float64, recorded only)", F16 + TAG, far, 0.0, float("inf"))
    print(f"hard {name} d{d}: max|gpu - float64| = {far:.2e} (recorded only)")
    if name == "underflow":
        assert not ref.any() and not got.any()
        Q, K, V = cr.zero_v_inputs(d, c.h, c.N, c.B)
        assert not causal(F16, dev, Q, K, V, c.h * d, c.h).any()


@pytest.mark.parametrize("variant,d", [(INT8, 32), (INT8, 64), (INT8, 128), (F16, 64), (F16, 128)])
def test_rows_before_the_spike_tile_are_bit_identical(dev, variant, d):
    """Keys 160..191 are one key tile and one quantisation group: rows < 160 never visit it (a wave whose diagonal
    lies earlier skips the tile body) and equal the run without the spike bit for bit; every later row changes."""
    c = cr.HARD["spike_tile"]
    spike = causal(variant, dev, *cr.hard_inputs("spike_tile", d), c.h * d, c.h)
    plain = causal(variant, dev, *cr.hard_inputs("spike_tile", d, spike=False), c.h * d, c.h)
    assert np.array_equal(spike[:, :160], plain[:, :160])
    assert (spike[:, 160:] != plain[:, 160:]).any(axis=-1).all()


@pytest.mark.parametrize("variant,name,d", [(INT8,) + nd for nd in cr.HARD_INT8] + [(F16,) + nd for nd in cr.HARD_F16],
                         ids=str)
def test_hard_cases_repeat_and_split_by_batch(dev, variant, name, d):
    """A hard case run twice is bit-identical (N = 288: the second pass of an int8 q-block pair restarts from
    anchor = 0 after the first re-anchored); each sequence of a B = 2 case equals its own B = 1 call."""
    c = cr.HARD[name]
    t = to_dev(dev, *cr.hard_inputs(name, d))
    a = solve_opts(variant, t, c.h * d, c.h, CAUSAL)
    assert np.array_equal(a, solve_opts(variant, t, c.h * d, c.h, CAUSAL), equal_nan=True)
    for b in range(c.B if c.B > 1 else 0):
        one = solve_opts(variant, [x[b:b + 1].contiguous() for x in t], c.h * d, c.h, CAUSAL)
        assert np.array_equal(one[0], a[b], equal_nan=True)


# ---- the mask itself ------------------------------------------------------------------------------------
NEG_SHAPE = (160, 128, 2)  # N, d_model, h


@functools.lru_cache(maxsize=None)
def neg_inputs():
    return tuple(x for x in cr.inputs(NEG_SHAPE[0], NEG_SHAPE[1], 1, "normal", 120))


@pytest.mark.parametrize("variant", [INT8, F16])
@pytest.mark.parametrize("k", [0, 1, 3])
def test_negated_future_does_not_reach_the_past(dev, variant, k):
    """K and V negated from row j0 = 32 k + 13 on (a sign flip keeps every group's absmax, so no scale and no
    earlier byte changes; finite values only).  Rows below group k: bit-identical.  Rows of group k below j0
    share the diagonal tile -- and, for int8, its one sP -- with changed rows: within the variant's tolerance
    of the reference on the changed input.  Rows from j0 on differ."""
    from oracle import oracle
    N, d_model, h = NEG_SHAPE
    Q, K, V = neg_inputs()
    j0 = 32 * k + 13
    K2, V2 = K.copy(), V.copy()
    K2[:, j0:] *= -1
    V2[:, j0:] *= -1
    base = causal(variant, dev, Q, K, V, d_model, h)
    neg = causal(variant, dev, Q, K2, V2, d_model, h)
    assert np.array_equal(neg[:, :32 * k], base[:, :32 * k])
    rows = slice(32 * k, j0)
    if variant == INT8:
        ref, unit, _ = cr.fa_int8(oracle, Q, K2, V2, d_model, h, causal=True)
        assert_int8(f"negated future k={k}", neg[:, rows], ref[:, rows], cr.per_element(unit, d_model // h)[:, rows], TAG)
    else:
        ref = cr.attention_f64(Q, K2, V2, d_model, h, causal=True)
        assert_f16(f"negated future k={k}", neg[:, rows], ref[:, rows])
    assert (neg[:, j0:] != base[:, j0:]).any(axis=-1).all()


@pytest.mark.parametrize("variant,N,d_model,h", [(INT8, 96, 64, 2), (INT8, 160, 256, 2), (F16, 96, 128, 2),
                                                 (F16, 160, 256, 2)])
def test_row0_is_dequantised_v0(dev, oracle_mod, variant, N, d_model, h):
    """Row 0 attends key 0 alone, so it is V[0] as the variant holds it -- Vi[0] sV[0] for int8 (Pi = 127 and
    sP = 1/127 cancel), half(V[0]) for fp16 -- to 1e-6 relative.  That identity needs row 0's p to be exactly
    1: for int8 its p must be the tile's largest (one sP per tile; a row with a negative score has p < 1 while
    another row has p = 1, and Pi = rint(127 p) then carries up to 0.4 % rounding), for fp16 half(p) must
    equal p (2^-11 otherwise; the lazy base keeps m = 0).  A zero query row gives score 0 = m0 and p = 1 in
    both contracts, so the inputs carry one; what is tested is that no other key reaches row 0."""
    d = d_model // h
    Q, K, V = cr.inputs(N, d_model, 2, "normal", 130)
    Q[:, 0] = 0.0
    got = causal(variant, dev, Q, K, V, d_model, h)
    if variant == INT8:
        Vi, sV = oracle_mod.quantize_heads(V, d_model, h)
        want = (Vi[:, :, 0].astype(np.float32) * sV[:, :, 0, None]).reshape(2, d_model)
    else:
        want = V[:, 0].astype(np.float16).astype(np.float32)
    rel = np.abs(got[:, 0] - want) / np.maximum(np.abs(want), 1e-30)
    print(f"{variant} N{N} d{d}: row 0 max relative error {rel.max():.2e}")
    np.testing.assert_allclose(got[:, 0], want, rtol=1e-6, atol=0)


@pytest.mark.parametrize("variant", [INT8, F16])
def test_causal_differs_from_full_attention_in_every_head(dev, variant):
    N, d_model, h = 256, 256, 4
    t = to_dev(dev, *cr.inputs(N, d_model, 2, "uniform", 140))
    full = solve_opts(variant, t, d_model, h, 0).reshape(2, N, h, d_model // h)
    masked = solve_opts(variant, t, d_model, h, CAUSAL).reshape(2, N, h, d_model // h)
    assert (full != masked).any(axis=(1, 3)).all()
    # the last row attends every key in both: its values agree to the variant's tolerance
    assert np.abs(full[:, -1] - masked[:, -1]).max() <= (5e-3 if variant == INT8 else 1e-3)


@pytest.mark.parametrize("variant", [INT8, F16, "fa", "fa_tc_int8_pt"])
def test_flags_zero_is_qmha_solve_ex(dev, variant):
    from quantizedmha_amd import torch_ext
    N, d_model, h = 288, 128, 2
    t = to_dev(dev, *cr.inputs(N, d_model, 2, "normal", 150))
    ex = torch_ext.flash_solve(t[0], t[1], t[2], d_model, h, kernel=variant)
    torch.cuda.synchronize()
    assert np.array_equal(solve_opts(variant, t, d_model, h, 0), ex.cpu().numpy())


# ---- robustness ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant,d_model,h", [(INT8, 64, 2), (INT8, 128, 2), (INT8, 256, 2), (F16, 128, 2), (F16, 256, 2)])
def test_repeatable_and_batch_independent(dev, variant, d_model, h):
    """The same call twice is bit-identical; a B = 2 call is bit-identical to two B = 1 calls."""
    N = 288
    Q, K, V = cr.inputs(N, d_model, 2, "normal", 160 + d_model)
    t = to_dev(dev, Q, K, V)
    a = solve_opts(variant, t, d_model, h, CAUSAL)
    assert np.array_equal(a, solve_opts(variant, t, d_model, h, CAUSAL))
    for b in range(2):
        one = solve_opts(variant, [x[b:b + 1].contiguous() for x in t], d_model, h, CAUSAL)
        assert np.array_equal(one[0], a[b])


@pytest.mark.parametrize("variant", [INT8, F16])
def test_caller_workspace_on_a_side_stream(dev, variant):
    """qmha_solve_opts with caller-owned scratch (the qmha_solve_ws rules) on a non-default stream equals the
    library-owned form; a workspace that is too small is refused."""
    from quantizedmha_amd import _lib
    lib = _lib.load()
    N, d_model, h, B = 160, 256, 2, 2
    t = to_dev(dev, *cr.inputs(N, d_model, B, "uniform", 170))
    want = solve_opts(variant, t, d_model, h, CAUSAL)
    need = lib.qmha_workspace_size(B, N, d_model, h, _lib.VARIANTS[variant])
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    got = solve_opts(variant, t, d_model, h, CAUSAL, ws=ws, stream=s.cuda_stream)
    assert np.array_equal(got, want)
    solve_opts(variant, t, d_model, h, CAUSAL, ws=ws[:need // 2], stream=s.cuda_stream, expect=1)


@pytest.mark.parametrize("variant,d_model,h", [("fa", 128, 2), ("unfused", 128, 2), ("fa_mfma", 128, 2),
                                               ("fa_tc_int8_pt", 128, 2), (INT8, 192, 2), (F16, 64, 2)])
def test_unsupported_causal_touches_nothing(dev, variant, d_model, h):
    from quantizedmha_amd import _lib
    t = to_dev(dev, *cr.inputs(64, d_model, 1, "normal", 180))
    got = solve_opts(variant, t, d_model, h, CAUSAL, expect=4)
    assert (got == GUARD).all()
    msg = _lib.load().qmha_last_error().decode()
    assert variant in msg and f"d = {d_model // h}" in msg


# ---- bindings and driver --------------------------------------------------------------------------------
def test_bindings_route_to_the_causal_kernels(dev):
    """torch_ext.flash_solve(causal=True) (the Python mirror, with out=, and the compiled module), the JAX
    raw-pointer entry and the batch-shard path give the C-ABI's result bit for bit."""
    from quantizedmha_amd import jax_ext, shard, torch_ext
    N, d_model, h = 96, 128, 2
    t = to_dev(dev, *cr.inputs(N, d_model, 2, "normal", 190))
    for variant in (INT8, F16):
        want = solve_opts(variant, t, d_model, h, CAUSAL)
        out = torch.empty_like(t[0])
        got = torch_ext.flash_solve(t[0], t[1], t[2], d_model, h, variant, out=out, causal=True)
        torch.cuda.synchronize()
        assert got is out and np.array_equal(out.cpu().numpy(), want)
        sharded = shard.solve_sharded(t[0], t[1], t[2], d_model, h, kernel=variant, causal=True)
        torch.cuda.synchronize()
        assert np.array_equal(sharded.cpu().numpy(), want)
        one = torch.empty_like(t[0][0])
        jax_ext.flash_solve(t[0][0].data_ptr(), t[1][0].data_ptr(), t[2][0].data_ptr(), one.data_ptr(), N, d_model, h,
                            variant, causal=True)
        assert np.array_equal(one.cpu().numpy(), want[0])
    got = compiled_module().flash_solve(t[0], t[1], t[2], d_model, h, INT8, causal=True)
    torch.cuda.synchronize()
    assert np.array_equal(got.cpu().numpy(), solve_opts(INT8, t, d_model, h, CAUSAL))
    with pytest.raises(RuntimeError, match="not supported"):
        torch_ext.flash_solve(t[0], t[1], t[2], d_model, h, "fa", causal=True)


@pytest.mark.parametrize("variant", [INT8, F16])
def test_driver_causal_flag(dev, variant, tmp_path):
    """qmha_profile --causal: the all-ones check (every row still 1) and the random-data check against the
    driver's own masked CPU attention pass, and --json says so."""
    exe = os.path.join(ROOT, "quantizedmha_amd", "bin", "qmha_profile")
    r = subprocess.run([exe, f"--kernel={variant}", "--causal", "--N=256", "--d_model=128", "--h=2", "--warmup=1",
                        "--runs=1", "--check-random", "--json", "--threads=4", f"--cache-dir={tmp_path}"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Correctness check PASSED" in r.stdout
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert line["causal"] is True and line["check"] == "passed" and line["check_random"] == "passed"
