"""CPU tests of the causal feature: the numpy restatement the GPU tests use as their int8
reference (tests/causal_ref.py) is held to the C oracle and to float64 masked attention, the C-ABI's flag
checks fail before any launch, and the bindings accept `causal=`.  The fp16 contract restated with the mask
(causal_ref.fa_fp16_lazy) is held to the C oracle's fa_fp16_lazy; the hard cases are shown to reach the int8
re-anchor and the fp16 rebase, closed forms guard both restatements, and two wrong masks are shown to land far
outside the GPU tests' bounds.  No kernel is launched here."""
import ctypes
import functools
import inspect

import numpy as np
import pytest

from tests import causal_ref as cr

ALL_INT8_CASES = cr.CASES + cr.CASES_INT8_D32


@pytest.fixture(scope="module")
def built():
    from tools.build import build
    build(verbose=False)
    return True


@pytest.mark.parametrize("N,d_model,h,B,dist,seed", ALL_INT8_CASES)
def test_restatement_equals_oracle_without_mask(oracle_mod, N, d_model, h, B, dist, seed):
    """causal=False is the C oracle (oracle/qmha_oracle.c fa_int8_item) up to numpy's exp against libm's
    expf: every element within two one-flip units + 5e-5, the bound the GPU is held to."""
    Q, K, V = cr.inputs(N, d_model, B, dist, seed)
    got, unit, _ = cr.fa_int8(oracle_mod, Q, K, V, d_model, h, causal=False)
    ref = oracle_mod.fa_int8(Q, K, V, d_model, h)
    err = np.abs(got.astype(np.float64) - ref)
    tol = 2.0 * cr.per_element(unit, d_model // h) + 5e-5
    print(f"N={N} d={d_model // h}: max|restatement - oracle| = {err.max():.2e}, worst err/tol = {(err / tol).max():.3f}")
    assert (err <= tol).all(), (float(err.max()), float((err / tol).max()))


@pytest.mark.parametrize("N,d_model,h,B,dist,seed", ALL_INT8_CASES)
def test_causal_restatement_within_quantisation_budget(oracle_mod, N, d_model, h, B, dist, seed):
    """causal=True against float64 masked attention.  Rows >= 32: the project's 5e-3 int8 budget.  Rows < 32
    average so few keys (row 0: one) that V's own quantisation step shows: within 1.5 steps of V's first
    group, 1.5 * absmax(V_head[0:32]) / 127 -- a property of the contract, not of a kernel."""
    d = d_model // h
    Q, K, V = cr.inputs(N, d_model, B, dist, seed)
    got, _, _ = cr.fa_int8(oracle_mod, Q, K, V, d_model, h, causal=True)
    err = np.abs(got - cr.attention_f64(Q, K, V, d_model, h, causal=True))
    step = np.abs(V.reshape(B, N, h, d)[:, :32]).max(axis=(1, 3)) / 127.0  # [B, h]
    early = (err[:, :32].reshape(B, 32, h, d) / step[:, None, :, None]).max()
    late = err[:, 32:].max() if N > 32 else 0.0
    print(f"N={N} d={d}: rows >= 32 max err {late:.2e}; rows < 32 worst {early:.2f} V steps")
    assert late <= 5e-3, late
    assert early <= 1.5, early


def test_mask_semantics_of_the_restatement(oracle_mod):
    """Row 0 sees key 0 alone: the dequantised V[0] when its p is the tile's largest (Pi = 127 and
    sP = 1/127 cancel), which a zero query row makes certain (score 0 = m0, p = 1; with a negative score
    p < 1 while another row of the tile has p = 1, and Pi = rint(127 p) carries up to 0.4 % rounding).
    Negating K and V from row j0 on -- no absmax, so no scale and no earlier byte, changes -- leaves every
    row < j0 bit-identical."""
    N, d_model, h = 96, 64, 2
    d = d_model // h
    Q, K, V = cr.inputs(N, d_model, 1, "normal", 7)
    Q[:, 0] = 0.0
    base, _, _ = cr.fa_int8(oracle_mod, Q, K, V, d_model, h, causal=True)
    Vi, sV = oracle_mod.quantize_heads(V, d_model, h)
    for k in range(h):
        np.testing.assert_allclose(base[0, 0, k * d:(k + 1) * d], Vi[0, k, 0].astype(np.float32) * sV[0, k, 0], rtol=1e-6)
    j0 = 45
    K2, V2 = K.copy(), V.copy()
    K2[:, j0:] *= -1
    V2[:, j0:] *= -1
    neg, _, _ = cr.fa_int8(oracle_mod, Q, K2, V2, d_model, h, causal=True)
    assert np.array_equal(neg[:, :j0], base[:, :j0])
    assert (neg[:, j0:] != base[:, j0:]).any(axis=-1).all()


# ---- the fp16 contract restated (cr.fa_fp16_lazy) -------------------------------------------------------
F16_CASES = [c for c in cr.CASES if c[1] // c[2] in (64, 128)] + cr.CASES_F16_EXTRA
MUTANTS = ("mask_after_max", "leak_next")


@functools.lru_cache(maxsize=None)
def hard_int8(name, d, base2=True, mutant=None, **kw):
    """(Q, K, V, O, per-element one-flip unit, Rise) of a hard case, computed once and shared (read-only)."""
    from oracle import oracle
    c = cr.HARD[name]
    Q, K, V = cr.hard_inputs(name, d, **kw)
    out, unit, rise = cr.fa_int8(oracle, Q, K, V, c.h * d, c.h, causal=True, base2=base2, _mutant=mutant)
    return Q, K, V, out, cr.per_element(unit, d), rise


@functools.lru_cache(maxsize=None)
def hard_f16(name, d, mutant=None, **kw):
    """(Q, K, V, O, rebased, rebased on a diagonal tile) of a hard case under the fp16 contract, shared."""
    c = cr.HARD[name]
    Q, K, V = cr.hard_inputs(name, d, **kw)
    return (Q, K, V) + cr.fa_fp16_lazy(None, Q, K, V, c.h * d, c.h, causal=True, _mutant=mutant)


@pytest.mark.parametrize("N,d_model,h,B,dist,seed", F16_CASES)
def test_lazy_restatement_equals_oracle_without_mask(oracle_mod, N, d_model, h, B, dist, seed):
    """causal=False is oracle.fa_fp16_lazy (qmha_oracle.c fa_fp16_lazy_item) up to numpy's exp2 against libm's
    exp2f: within fp16_lazy_tol(N), the bound the GPU is held to against that contract (measured <= 5.2e-6).
    These benign inputs never rebase, masked or not -- the branch the hard cases below exist for."""
    Q, K, V = cr.inputs(N, d_model, B, dist, seed)
    got, rebased, _ = cr.fa_fp16_lazy(oracle_mod, Q, K, V, d_model, h)
    err = float(np.abs(got.astype(np.float64) - oracle_mod.fa_fp16_lazy(Q, K, V, d_model, h)).max())
    print(f"N={N} d={d_model // h}: max|restatement - oracle| = {err:.2e} (bound {cr.fp16_lazy_tol(N):.0e})")
    assert err <= cr.fp16_lazy_tol(N), err
    assert rebased == 0


@pytest.mark.parametrize("N,d_model,h,B,dist,seed", F16_CASES)
def test_causal_lazy_restatement_vs_float64(oracle_mod, N, d_model, h, B, dist, seed):
    """causal=True against float64 masked attention within verify.cu's max(1e-3, 1e-3 |ref|), the bound the GPU
    kernel is held to (measured worst 7.6e-4); 0 rebased rows on every committed case."""
    Q, K, V = cr.inputs(N, d_model, B, dist, seed)
    got, rebased, on_diag = cr.fa_fp16_lazy(oracle_mod, Q, K, V, d_model, h, causal=True)
    ref = cr.attention_f64(Q, K, V, d_model, h, causal=True)
    print(f"N={N} d={d_model // h}: max|causal restatement - float64| = {np.abs(got - ref).max():.2e}")
    assert oracle_mod.verify_results(got, ref.astype(np.float32), 1e-3, 1e-3) == -1
    assert (rebased, on_diag) == (0, 0)


@pytest.mark.parametrize("d", cr.HARD["staircase"].f16_d)
def test_lazy_restatement_equals_oracle_on_the_staircase(oracle_mod, d):
    """Rebasing inputs, no mask: within 2^-10 max|V| of the C oracle, test_lazy_base_staircase's flip bound
    (two dominant keys per row with p ~ 2^11.4: an exp2 ulp flips half(p)).  Measured 3.5e-6 (d = 64) and
    1.0e-3 (d = 128) against 4.2e-3."""
    c = cr.HARD["staircase"]
    Q, K, V = cr.hard_inputs("staircase", d)
    got, rebased, _ = cr.fa_fp16_lazy(oracle_mod, Q, K, V, c.h * d, c.h)
    err = float(np.abs(got.astype(np.float64) - oracle_mod.fa_fp16_lazy(Q, K, V, c.h * d, c.h)).max())
    tol = 2.0 ** -10 * float(np.abs(V).max())
    print(f"staircase d={d}: max|restatement - oracle| = {err:.2e} (bound {tol:.2e}), {rebased} rebased (row, tile) pairs")
    assert err <= tol, (err, tol)
    assert rebased > 0


# ---- every hard case reaches the branch it was built for -----------------------------------------------
# int8: where the kernel's re-anchor (m_new - anchor > 48, any row of the wave) must fire, from the inputs alone:
#   const       every score is 3.5^2 sqrt(d) log2 e = 100 / 141 / 200 units above m0 = 0 on tile 0 -- group 0's diagonal;
#   spike_tile  keys 160..191 score 6 sum(q) / sqrt(d) log2 e = 49 +- 2.6 / 69 / 98 units above the rest: group 5 meets
#               them on its diagonal, groups 6 and 7 off it;
#   ramp        the max climbs to 4 sqrt(d) 1.04 log2 e = 34 / 48 / 68 units, about 1/16 of it per tile: no single tile
#               rises by more than 6 units, the re-anchor fires on the accumulated distance, and only from d = 64 on.
# superdiag's strongest keys are the MASKED ones; the visible ones score 11.5 z log2 units, so a re-anchor there is
# chance (3 to 6 of 32 groups) and is not asserted: that case is for the mask (the mutant tests below).
ONE_TILE_RISE = {("const", 32), ("const", 64), ("const", 128), ("spike_tile", 32), ("spike_tile", 64), ("spike_tile", 128)}
REANCHORS = ONE_TILE_RISE | {("ramp", 64), ("ramp", 128)}
REANCHORS_ON_DIAG = REANCHORS
ONE_TILE_RISE_ON_DIAG = ONE_TILE_RISE  # const: group 0 on tile 0; spike_tile: group 5 on tile 5


@pytest.mark.parametrize("name,d", cr.HARD_INT8)
@pytest.mark.parametrize("base2", [True, False])
def test_int8_hard_cases_reach_the_reanchor(oracle_mod, name, d, base2):
    _, _, _, out, _, rise = hard_int8(name, d, base2)
    big = rise.log2 > cr.REANCHOR
    groups = rise.anchored[:, ::cr.GROUP]
    print(f"{name} d={d} base2={base2}: largest one-tile rise {rise.log2.max():.1f} log2 units, {int(big.sum())} rows above "
          f"48 ({int((big & rise.diag).sum())} on their diagonal tile); {int((groups > 0).sum())} of {groups.size} groups "
          f"re-anchor, {int(rise.anchored_diag[:, ::cr.GROUP].sum())} on their diagonal tile")
    assert np.isfinite(out).all()
    if name != "superdiag":  # there a visible key 48 units up is chance (0 to 2 rows of 1024): recorded only
        assert big.any() == ((name, d) in ONE_TILE_RISE)
        assert (big & rise.diag).any() == ((name, d) in ONE_TILE_RISE_ON_DIAG)
    if (name, d) in REANCHORS:
        assert (rise.anchored > 0).any()
    if (name, d) in REANCHORS_ON_DIAG:
        assert rise.anchored_diag.any()
    if name in ("underflow", "zero_q", "nan_int8") or (name, d) == ("ramp", 32):
        assert not rise.anchored.any()


@pytest.mark.parametrize("name,d", cr.HARD_F16)
def test_fp16_hard_cases_reach_the_rebase(name, d):
    _, _, _, out, rebased, on_diag = hard_f16(name, d)
    print(f"{name} d={d}: {rebased} rebased (row, tile) pairs, {on_diag} on a diagonal tile")
    assert np.isfinite(out).all()
    if name in ("const", "superdiag", "ramp", "spike_tile", "staircase"):
        assert rebased > 0 and on_diag > 0
    else:
        assert (rebased, on_diag) == (0, 0)


@pytest.mark.parametrize("N,d_model,h,B,dist,seed", ALL_INT8_CASES)
def test_committed_cases_never_reanchor_and_base2_agrees(oracle_mod, N, d_model, h, B, dist, seed):
    """The benign cases: no re-anchor, no one-tile rise above 6 log2 units; and the kernel's base-2 score
    arithmetic (base2=True, the GPU's reference on the hard cases) agrees with the oracle's nats within the
    GPU bound 2 u_r + 5e-5 (measured <= 0.29 unit)."""
    Q, K, V = cr.inputs(N, d_model, B, dist, seed)
    nats, unit, rise_n = cr.fa_int8(oracle_mod, Q, K, V, d_model, h, causal=True)
    two, _, rise_2 = cr.fa_int8(oracle_mod, Q, K, V, d_model, h, causal=True, base2=True)
    for rise in (rise_n, rise_2):
        assert not rise.anchored.any() and rise.log2.max() < 6.0
    err = np.abs(two.astype(np.float64) - nats)
    pe = cr.per_element(unit, d_model // h)
    print(f"N={N} d={d_model // h}: base2 vs nats {cr.flip_units(err, pe):.2f} one-flip units (bound 2)")
    assert (err <= 2.0 * pe + 5e-5).all()


@pytest.mark.parametrize("name,d", cr.HARD_INT8)
def test_base2_vs_nats_on_the_hard_cases_is_recorded(oracle_mod, name, d):
    """Not asserted: at 50..200 log2 units the two statements of the score differ by ~1e-5 in the exponent, which
    can flip a Pi (measured 0 to 0.98 unit).  Both must stay finite."""
    _, _, _, two, pe, _ = hard_int8(name, d, True)
    nats = hard_int8(name, d, False)[3]
    print(f"{name} d={d}: base2 vs nats {cr.flip_units(np.abs(two.astype(np.float64) - nats), pe):.2f} one-flip units")
    assert np.isfinite(two).all() and np.isfinite(nats).all()


# ---- closed forms: they guard the restatements themselves -------------------------------------------------
def dequantised_v(oracle_mod, V, d_model, h):
    Vi, sV = oracle_mod.quantize_heads(V, d_model, h)  # [B, h, N, d], [B, h, N / 32]
    deq = Vi.astype(np.float32) * np.repeat(sV, cr.GROUP, axis=2)[..., None]
    return deq.transpose(0, 2, 1, 3).reshape(V.shape)


# 4 x the error measured on the CPU (float32 rounding only; the margin is for libm differences): DESIGN.md 10.3
INT8_CLOSED = {("const", True): 4 * 2.4e-7, ("const", False): 4 * 1.2e-7, ("zero_q", True): 4 * 9.0e-8,
               ("zero_q", False): 4 * 9.0e-8}
F16_CLOSED = {("const", 64): 4 * 4.8e-6, ("const", 128): 4 * 1.3e-5, ("zero_q", 128): 4 * 5.3e-8}


@pytest.mark.parametrize("name,d", [nd for nd in cr.HARD_INT8 if nd[0] in ("const", "zero_q")])
@pytest.mark.parametrize("base2", [True, False])
def test_int8_equal_scores_give_the_prefix_mean_of_dequantised_v(oracle_mod, name, d, base2):
    """All visible scores of a row equal (const: 100..200 log2 units, zero_q: 0): every visible p is 1, every
    visible Pi 127 with sP = 1/127, and row r is the mean of Vi sV over keys 0..r."""
    c = cr.HARD[name]
    _, _, V, out, _, _ = hard_int8(name, d, base2)
    err = float(np.abs(out - cr.prefix_mean(dequantised_v(oracle_mod, V, c.h * d, c.h))).max())
    print(f"{name} d={d} base2={base2}: max|restatement - prefix mean| = {err:.2e} (bound {INT8_CLOSED[name, base2]:.1e})")
    assert err <= INT8_CLOSED[name, base2], err


@pytest.mark.parametrize("name,d", [nd for nd in cr.HARD_F16 if nd[0] in ("const", "zero_q")])
def test_fp16_equal_scores_give_the_prefix_mean_of_half_v(name, d):
    """const: after the rebase p = exp2(fma(S, c, -RN(S c))) = 1 + O(2^-17), half(p) = 1 while l sums the
    unrounded p -- that relative 5e-6 is the whole error."""
    _, _, V, out, _, _ = hard_f16(name, d)
    err = float(np.abs(out - cr.prefix_mean(V.astype(np.float16))).max())
    print(f"{name} d={d}: max|restatement - prefix mean| = {err:.2e} (bound {F16_CLOSED[name, d]:.1e})")
    assert err <= F16_CLOSED[name, d], err


def test_underflow_is_exactly_zero(oracle_mod):
    """Every score ~ -100 log2 units below m0 = 0: l stays under both guards and every restatement writes 0;
    V = 0 gives 0 whatever the scores."""
    for base2 in (True, False):
        assert not hard_int8("underflow", 64, base2)[3].any()
    assert not hard_f16("underflow", 64)[3].any()
    c = cr.HARD["underflow"]
    Q, K, V = cr.zero_v_inputs(64, c.h, c.N, c.B)
    assert not cr.fa_int8(oracle_mod, Q, K, V, c.h * 64, c.h, causal=True, base2=True)[0].any()
    assert not cr.fa_fp16_lazy(oracle_mod, Q, K, V, c.h * 64, c.h, causal=True)[0].any()


@pytest.mark.parametrize("d", [32, 64, 128])
def test_rows_before_the_spike_do_not_see_it(oracle_mod, d):
    """Keys 160..191 are one key tile and one quantisation group: rows < 160 never visit it, and are bit-identical
    to the same inputs without the spike in every restatement; group 5 (its diagonal) and later rows change."""
    for base2 in (True, False):
        spike, plain = hard_int8("spike_tile", d, base2)[3], hard_int8("spike_tile", d, base2, spike=False)[3]
        assert np.array_equal(spike[:, :160], plain[:, :160])
        assert (spike[:, 160:] != plain[:, 160:]).any(axis=-1).all()
    if d in cr.HARD["spike_tile"].f16_d:
        spike, plain = hard_f16("spike_tile", d)[3], hard_f16("spike_tile", d, spike=False)[3]
        assert np.array_equal(spike[:, :160], plain[:, :160])
        assert (spike[:, 160:] != plain[:, 160:]).any(axis=-1).all()


# ---- the tests can fail: two wrong masks ------------------------------------------------------------------
@pytest.mark.parametrize("mutant", MUTANTS)
@pytest.mark.parametrize("d", [32, 64, 128])
@pytest.mark.parametrize("base2", [True, False])
def test_int8_mask_mutants_are_far_outside_the_gpu_bound_on_superdiag(oracle_mod, mutant, d, base2):
    """K[r + 1] = 32 Q[r]: the first masked key of every row scores 65..130 log2 units above the visible ones.  A
    mask applied after the row max, or one key late, moves the output by >= 10 x the GPU bound of 2 one-flip
    units (measured 168..191 and 425..490 units)."""
    _, _, _, ref, pe, _ = hard_int8("superdiag", d, base2)
    bad = hard_int8("superdiag", d, base2, mutant)[3]
    units = cr.flip_units(np.abs(bad.astype(np.float64) - ref), pe)
    print(f"superdiag d={d} base2={base2} {mutant}: {units:.0f} one-flip units from the correct mask")
    assert units >= 10 * 2.0, units


@pytest.mark.parametrize("mutant", MUTANTS)
@pytest.mark.parametrize("d", [64, 128])
def test_fp16_mask_mutants_are_far_outside_the_gpu_bound_on_superdiag(mutant, d):
    """The same for the fp16 contract against its GPU bound 2^-10 max|V| (measured 800..1360 x the bound):
    "mask_after_max" moves a rebasing row's base to a masked key's score and every visible p underflows."""
    _, _, V, ref, _, _ = hard_f16("superdiag", d)
    bad = hard_f16("superdiag", d, mutant)[3]
    tol = 2.0 ** -10 * float(np.abs(V).max())
    err = float(np.abs(bad - ref).max())
    print(f"superdiag d={d} {mutant}: {err / tol:.0f} x the GPU bound")
    assert err >= 10 * tol, (err, tol)


def test_benign_inputs_let_a_mask_after_the_max_through(oracle_mod):
    """The gap the hard cases close: on the committed N(0, 0.25) cases the "mask_after_max" mutant stays inside the
    GPU's 2-unit bound (1.59 at N = 32, 1.78 at N = 96, 1.94 at N = 256), so those cases alone could not tell."""
    under = []
    for N, d_model, h, B, dist, seed in [c for c in cr.CASES if c[4] == "normal" and c[0] <= 256]:
        Q, K, V = cr.inputs(N, d_model, B, dist, seed)
        ref, unit, _ = cr.fa_int8(oracle_mod, Q, K, V, d_model, h, causal=True)
        bad, _, _ = cr.fa_int8(oracle_mod, Q, K, V, d_model, h, causal=True, _mutant="mask_after_max")
        units = cr.flip_units(np.abs(bad.astype(np.float64) - ref), cr.per_element(unit, d_model // h))
        print(f"N={N} d={d_model // h}: mask_after_max moves the output by {units:.2f} one-flip units")
        under.append(units <= 2.0)
    assert any(under)


# ---- C-ABI argument checks: they fail before any launch, so no device is needed ------------------------
CAUSAL = 1
NOSYS_CASES = [  # (variant id, name, d_model, h)
    (0, "fa", 128, 2),
    (3, "unfused", 128, 2),
    (4, "fa_mfma", 128, 2),
    (5, "fa_tc_int8_pt", 128, 2),
    (2, "fa_tc_int8_b", 192, 2),  # d = 96
    (1, "fa_tc_v1a", 192, 2),     # d = 96
    (1, "fa_tc_v1a", 64, 2),      # d = 32: int8 only
    (2, "fa_tc_int8_b", 512, 2),  # d = 256
]


def test_unknown_flag_bits_are_invalid(built):
    from quantizedmha_amd import _lib
    lib = _lib.load()
    dummy = ctypes.c_void_p(0x1000)  # never dereferenced: checks run first
    for flags in (2, 3, 0x80000000):
        st = lib.qmha_solve_opts(dummy, dummy, dummy, dummy, 1, 128, 128, 2, 2, flags, None, 0, None)
        assert st == 1, (flags, st)
        assert "flag" in lib.qmha_last_error().decode()
    # the shape checks of qmha_solve_ex come first and still apply
    st = lib.qmha_solve_opts(dummy, dummy, dummy, dummy, 1, 100, 128, 2, 2, CAUSAL, None, 0, None)
    assert st == 1 and "multiple of 32" in lib.qmha_last_error().decode()


@pytest.mark.parametrize("vid,name,d_model,h", NOSYS_CASES)
def test_causal_unsupported_combinations_are_nosys(built, vid, name, d_model, h):
    from quantizedmha_amd import _lib
    lib = _lib.load()
    dummy = ctypes.c_void_p(0x1000)
    for ws in (None, dummy):  # library-owned and caller-owned workspace forms
        st = lib.qmha_solve_opts(dummy, dummy, dummy, dummy, 1, 128, d_model, h, vid, CAUSAL, ws, 1 << 30, None)
        assert st == 4, st
        msg = lib.qmha_last_error().decode()
        assert name in msg and f"d = {d_model // h}" in msg, msg


def test_python_bindings_accept_causal():
    """`causal` is the trailing keyword, default False, of every binding; reference call sites are unchanged."""
    from quantizedmha_amd import jax_binding, jax_ext, shard, torch_ext
    for fn in (torch_ext.flash_solve, jax_ext.flash_solve, jax_binding.flash_solve_jax, shard.solve_sharded,
               shard.solve_shard_gather):
        params = list(inspect.signature(fn).parameters.values())
        assert params[-1].name == "causal" and params[-1].default is False, fn
    assert [p.name for p in inspect.signature(torch_ext.flash_solve).parameters.values()][:6] == \
        ["Q", "K", "V", "d_model", "num_heads", "kernel"]


def test_torch_bindings_take_causal_and_still_work_without_it(built):
    """Both torch bindings reach their own argument checks with and without `causal` (a binding that did
    not know the keyword would raise TypeError instead)."""
    torch = pytest.importorskip("torch")
    from quantizedmha_amd import torch_ext
    from tests.gpu_support import compiled_module
    q = torch.zeros(32, 32)
    for kw in ({}, {"causal": True}, {"causal": False}):
        with pytest.raises(RuntimeError, match="Inputs must be CUDA tensors"):
            torch_ext.flash_solve(q, q, q, 32, 1, **kw)
    compiled = compiled_module()
    assert "causal" in compiled.flash_solve.__doc__
    for kw in ({}, {"causal": True}, {"kernel": "fa_tc_v1a", "causal": True}):
        with pytest.raises(RuntimeError, match="Inputs must be CUDA tensors"):
            compiled.flash_solve(q, q, q, 32, 1, **kw)


def test_shard_passes_causal_to_the_solve():
    """The batch-shard path hands `causal=True` to the solve (here a CPU stand-in that honours it) and leaves
    a stand-in without the keyword alone when the flag is off.  Single process: the mask is per sequence, so
    sharding the batch does not interact with it (the gloo tests of tests/test_dist.py cover the exchange)."""
    torch = pytest.importorskip("torch")
    from quantizedmha_amd import shard
    Q, K, V = (torch.from_numpy(x) for x in cr.inputs(64, 64, 2, "normal", 5))

    def stand_in(q, k, v, d_model, h, kernel, causal=False):
        return torch.from_numpy(cr.attention_f64(q.numpy(), k.numpy(), v.numpy(), d_model, h, causal)).float()

    def old_stand_in(q, k, v, d_model, h, kernel):
        return stand_in(q, k, v, d_model, h, kernel)

    full = shard.solve_sharded(Q, K, V, 64, 2, solve_fn=stand_in)
    masked = shard.solve_sharded(Q, K, V, 64, 2, solve_fn=stand_in, causal=True)
    assert torch.equal(full, shard.solve_sharded(Q, K, V, 64, 2, solve_fn=old_stand_in))
    assert torch.equal(masked, stand_in(Q, K, V, 64, 2, "fa_tc_int8_b", causal=True))
    assert not torch.equal(masked, full)
    out = torch.empty_like(Q)
    shard.solve_shard_gather(Q, K, V, 64, 2, batch=2, solve_fn=stand_in, out=out, causal=True)
    assert torch.equal(out, masked)
