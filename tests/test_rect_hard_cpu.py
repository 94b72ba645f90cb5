"""CPU tests of the rectangular hard cases: rect_ref.HARD_SHAPES cut causal_ref's hard inputs to
rectangles that drive the int8 re-anchor, the fp16 rebase and the guards of qmha_fa_masked.hip's rectangular
instances, with and without the mask.

Held here, with no kernel launched:
  * every shape reaches the branch it is listed for -- counts asserted exactly where the input's construction
    fixes them, recorded where they are chance;
  * a causal rectangular reference on hard inputs is, exactly, the last Nq rows of the square hard problem at N = Nk;
  * closed forms (equal scores give a mean of V; underflow and V = 0 give exactly 0) guard the references;
  * the GPU tests can fail: a re-anchor or a rebase that leaves l or O unscaled ("stale_l", "stale_o") lands
    hundreds of times outside the GPU bounds on `spike_tile`, and does not move `const` at all -- there the only
    rise is on the first tile, where O = l = 0, so `const` tests the overflow a MISSING re-anchor would cause and
    `spike_tile` the rescale itself.  Both are needed.
"""
import functools

import numpy as np
import pytest

from tests import causal_ref as cr
from tests import rect_ref as rr

_ids = rr.hard_id
CAUSAL_INT8 = [sd for sd in rr.HARD_INT8 if sd[0].causal]
CAUSAL_F16 = [sd for sd in rr.HARD_F16 if sd[0].causal]


def shape_of(name, Nq, Nk, causal):
    return next(s for s in rr.HARD_SHAPES if (s.name, s.Nq, s.Nk, s.causal) == (name, Nq, Nk, causal))


SPIKE_CAUSAL, SPIKE_FULL = shape_of("spike_tile", 160, 256, True), shape_of("spike_tile", 64, 256, False)
CONST_CAUSAL, CONST_FULL = shape_of("const", 288, 352, True), shape_of("const", 160, 96, False)


@functools.lru_cache(maxsize=None)
def hard_int8(shape, d, base2=True, mutant=None, **kw):
    """(Q, K, V, O, per-element one-flip unit, Rise) of a hard shape, computed once and shared (read-only)."""
    from oracle import oracle
    c = cr.HARD[shape.name]
    Q, K, V = rr.hard_inputs(shape.name, d, shape.Nq, shape.Nk, **kw)
    out, unit, rise = rr.fa_int8(oracle, Q, K, V, c.h * d, c.h, causal=shape.causal, base2=base2, _mutant=mutant, stats=True)
    return Q, K, V, out, cr.per_element(unit, d), rise


@functools.lru_cache(maxsize=None)
def hard_f16(shape, d, mutant=None, **kw):
    """(Q, K, V, O, rebased (row, tile) pairs, those on a diagonal tile) under the fp16 contract, shared."""
    c = cr.HARD[shape.name]
    Q, K, V = rr.hard_inputs(shape.name, d, shape.Nq, shape.Nk, **kw)
    return (Q, K, V) + rr.fa_fp16_lazy(None, Q, K, V, c.h * d, c.h, causal=shape.causal, _mutant=mutant, stats=True)


def test_hard_inputs_are_the_last_chunk_of_the_square_case():
    for name, d, Nq, Nk in (("spike_tile", 64, 160, 256), ("ramp", 32, 64, 512), ("zero_q", 128, 64, 96)):
        sq = cr.HARD[name].build(d, cr.HARD[name].h, Nk, cr.HARD[name].B)
        Q, K, V = rr.hard_inputs(name, d, Nq, Nk)
        assert Q.shape == (cr.HARD[name].B, Nq, cr.HARD[name].h * d) and K.shape == V.shape == sq[1].shape
        assert np.array_equal(Q, sq[0][:, Nk - Nq:]) and np.array_equal(K, sq[1]) and np.array_equal(V, sq[2])
        assert not np.shares_memory(Q, sq[0])
    Q, K, V = rr.hard_inputs("const", 32, 160, 96)  # Nq > Nk: built at N = Nq
    assert Q.shape[1] == 160 and K.shape[1] == V.shape[1] == 96


# ---- every shape reaches the branch it is listed for ------------------------------------------------------
# int8, per (shape, d): (groups that re-anchor, of them on their diagonal tile, rows rising > 48 units in one tile),
# groups counted over both heads (and both sequences of zero_q).  None: chance, recorded only.  What the
# construction fixes:
#   const       every score is 100 / 141 / 200 log2 units above m0 = 0 on tile 0, which no group of these shapes
#               has as its diagonal: every group re-anchors there, every row rises;
#   spike_tile  keys 160..191 score 49 +- 2.6 / 69 / 98 units above the rest.  (160, 256) causal: query groups 0, 1
#               never reach them, group 2 meets them on its diagonal, 3 and 4 off it.  Non-causal: every group,
#               after four (one: Nq > Nk has Gk = 7, the spike in its stage 2) ordinary stages.  At d = 32 the rise
#               straddles 48, so the row count is chance; one row above 48 re-anchors its group;
#   ramp        at most 6 units per tile: no row rises by 48, the re-anchor fires on the accumulated distance --
#               34 units in all at d = 32 (none), 48 at d = 64 (chance: recorded, at least one asserted), 68 at
#               d = 128 (every group: these shapes' groups all see the whole ramp).
INT8_COUNTS = {
    ("const", 288, 352, True): {32: (18, 0, 576), 64: (18, 0, 576), 128: (18, 0, 576)},
    ("spike_tile", 160, 256, True): {32: (6, 2, None), 64: (6, 2, 192), 128: (6, 2, 192)},
    ("ramp", 64, 512, True): {32: (0, 0, 0), 64: (None, None, 0), 128: (4, None, 0)},
    ("spike_tile", 64, 256, False): {32: (4, 0, None), 64: (4, 0, 128), 128: (4, 0, 128)},
    ("spike_tile", 288, 224, False): {32: (18, 0, None), 64: (18, 0, 576), 128: (18, 0, 576)},
    ("const", 160, 96, False): {32: (10, 0, 320), 64: (10, 0, 320), 128: (10, 0, 320)},
    ("ramp", 32, 512, False): {32: (0, 0, 0), 64: (None, 0, 0), 128: (2, 0, 0)},
}
QUIET = (0, 0, 0)  # underflow, zero_q, nan_int8: the guards' cases take no branch


@pytest.mark.parametrize("shape,d", rr.HARD_INT8, ids=_ids)
@pytest.mark.parametrize("base2", [True, False])
def test_int8_hard_shapes_reach_the_reanchor(oracle_mod, shape, d, base2):
    _, _, _, out, _, rise = hard_int8(shape, d, base2)
    groups, on_diag = rise.anchored[:, ::cr.GROUP] > 0, rise.anchored_diag[:, ::cr.GROUP]
    big = rise.log2 > cr.REANCHOR
    got = (int(groups.sum()), int(on_diag.sum()), int(big.sum()))
    print(f"{rr.hard_id(shape)} d={d} base2={base2}: {got[0]} of {groups.size} groups re-anchor ({got[1]} on their diagonal "
          f"tile), {got[2]} rows rise > 48 in one tile ({int((big & rise.diag).sum())} on it), largest {rise.log2.max():.1f}")
    assert np.isfinite(out).all() and out.shape == (cr.HARD[shape.name].B, shape.Nq, cr.HARD[shape.name].h * d)
    want = INT8_COUNTS.get(shape[:4], {}).get(d, QUIET)
    for g, w in zip(got, want):
        assert w is None or g == w, (got, want)
    if shape.name == "spike_tile":
        assert 0 < got[2] <= 32 * got[0]
    if (shape.name, d) == ("ramp", 64):
        assert got[0] > 0 and (got[1] > 0) == shape.causal
    if not shape.causal:
        assert not rise.anchored_diag.any() and not rise.diag.any()


# fp16: (rebased (row, tile) pairs, of them on a diagonal tile).  const: every row, once, on tile 0.  spike_tile: every
# row that sees the spike, once (the 64 diagonal ones: query group 2, both heads).  ramp: chance, recorded.  staircase:
# each tile's two leading keys (in different key quarters) stand 11.4 log2 units above the last tile's, 2^11.4 < 4096 <
# 2^22.8: a row rebases on every second tile it visits, (tiles - 1) // 2 times.
F16_COUNTS = {
    ("const", 288, 352, True): (576, 0), ("spike_tile", 160, 256, True): (192, 64),
    ("spike_tile", 64, 256, False): (128, 0), ("spike_tile", 288, 224, False): (576, 0),
    ("const", 160, 96, False): (320, 0),
}


@pytest.mark.parametrize("shape,d", rr.HARD_F16, ids=_ids)
def test_fp16_hard_shapes_reach_the_rebase(shape, d):
    _, _, _, out, rebased, on_diag = hard_f16(shape, d)
    print(f"{rr.hard_id(shape)} d={d}: {rebased} rebased (row, tile) pairs, {on_diag} on a diagonal tile")
    assert np.isfinite(out).all()
    if shape[:4] in F16_COUNTS:
        assert (rebased, on_diag) == F16_COUNTS[shape[:4]]
    elif shape.name in ("ramp", "staircase"):
        assert rebased > 0 and (on_diag > 0) == shape.causal
        if shape.name == "staircase":
            h, Gk, Gq = cr.HARD[shape.name].h, shape.Nk // 32, shape.Nq // 32
            tiles = [min(g + Gk - Gq, Gk - 1) + 1 if shape.causal else Gk for g in range(Gq)]
            assert rebased == h * 32 * sum((t - 1) // 2 for t in tiles), (rebased, tiles)
    else:
        assert (rebased, on_diag) == (0, 0)


# ---- the construction, on hard inputs -----------------------------------------------------------------------
@pytest.mark.parametrize("shape,d", CAUSAL_INT8, ids=_ids)
def test_int8_causal_rect_is_the_last_rows_of_the_square_hard_case(oracle_mod, shape, d):
    c = cr.HARD[shape.name]
    sq = c.build(d, c.h, shape.Nk, c.B)
    for base2 in (True, False):
        want, unit, rise = cr.fa_int8(oracle_mod, *sq, c.h * d, c.h, causal=True, base2=base2)
        _, _, _, got, pe, got_rise = hard_int8(shape, d, base2)
        assert np.array_equal(got, want[:, -shape.Nq:], equal_nan=True)
        assert np.array_equal(pe, cr.per_element(unit, d)[:, -shape.Nq:])
        for mine, theirs in zip(got_rise, rise):
            assert np.array_equal(mine, theirs[:, -shape.Nq:])


@pytest.mark.parametrize("shape,d", CAUSAL_F16, ids=_ids)
def test_fp16_causal_rect_is_the_last_rows_of_the_square_hard_case(shape, d):
    c = cr.HARD[shape.name]
    want, n, nd = cr.fa_fp16_lazy(None, *c.build(d, c.h, shape.Nk, c.B), c.h * d, c.h, causal=True, per_row=True)
    _, _, _, got, rebased, on_diag = hard_f16(shape, d)
    assert np.array_equal(got, want[:, -shape.Nq:])
    assert (rebased, on_diag) == (int(n[:, -shape.Nq:].sum()), int(nd[:, -shape.Nq:].sum()))


def test_per_row_counts_sum_to_the_totals():
    c = cr.HARD["spike_tile"]
    Q, K, V = cr.hard_inputs("spike_tile", 64)
    out, n, nd = cr.fa_fp16_lazy(None, Q, K, V, c.h * 64, c.h, causal=True)
    out2, rows, rows_diag = cr.fa_fp16_lazy(None, Q, K, V, c.h * 64, c.h, causal=True, per_row=True)
    assert np.array_equal(out, out2) and (n, nd) == (int(rows.sum()), int(rows_diag.sum())) == (192, 64)
    assert rows.shape == (c.B, c.N, c.h) and not rows[:, :160].any() and (rows_diag[:, 160:192] == 1).all()


# ---- closed forms: they guard the references themselves -------------------------------------------------------
def dequantised_v(oracle_mod, V, d_model, h):
    Vi, sV = oracle_mod.quantize_heads(V, d_model, h)  # [B, h, Nk, d], [B, h, Nk / 32]
    deq = Vi.astype(np.float32) * np.repeat(sV, cr.GROUP, axis=2)[..., None]
    return deq.transpose(0, 2, 1, 3).reshape(V.shape)


def mean_of_visible(X, shape):
    """float64: causal, the mean of keys 0..r + Nk - Nq for row r; else the mean of all Nk keys, for every row."""
    X = np.asarray(X, np.float64)
    if shape.causal:
        return cr.prefix_mean(X)[:, shape.Nk - shape.Nq:]
    return np.broadcast_to(X.mean(axis=1, keepdims=True), (X.shape[0], shape.Nq, X.shape[2]))


# 4 x the largest error measured on the CPU over d and both score forms (float32 rounding only)
INT8_CLOSED = {("const", True): 4 * 5.9e-8, ("const", False): 4 * 3.2e-8, ("zero_q", True): 4 * 3.7e-8,
               ("zero_q", False): 4 * 2.5e-8}
F16_CLOSED = {("const", True, 64): 4 * 7.3e-7, ("const", True, 128): 4 * 1.9e-6, ("const", False, 64): 4 * 5.6e-7,
              ("const", False, 128): 4 * 1.3e-6, ("zero_q", True, 128): 4 * 2.9e-8, ("zero_q", False, 128): 4 * 1.3e-8}


@pytest.mark.parametrize("shape,d", [sd for sd in rr.HARD_INT8 if sd[0].name in ("const", "zero_q")], ids=_ids)
@pytest.mark.parametrize("base2", [True, False])
def test_int8_equal_scores_give_the_mean_of_dequantised_v(oracle_mod, shape, d, base2):
    """All visible scores of a row equal: every visible Pi is 127 with sP = 1 / 127, and the row is the mean of
    Vi sV over its visible keys -- from row Nk - Nq of the prefix mean on (causal) or over all Nk keys."""
    c = cr.HARD[shape.name]
    _, _, V, out, _, _ = hard_int8(shape, d, base2)
    err = float(np.abs(out - mean_of_visible(dequantised_v(oracle_mod, V, c.h * d, c.h), shape)).max())
    bound = INT8_CLOSED[shape.name, shape.causal]
    print(f"{rr.hard_id(shape)} d={d} base2={base2}: max|restatement - mean of V| = {err:.2e} (bound {bound:.1e})")
    assert err <= bound, err


@pytest.mark.parametrize("shape,d", [sd for sd in rr.HARD_F16 if sd[0].name in ("const", "zero_q")], ids=_ids)
def test_fp16_equal_scores_give_the_mean_of_half_v(shape, d):
    _, _, V, out, _, _ = hard_f16(shape, d)
    err = float(np.abs(out - mean_of_visible(V.astype(np.float16), shape)).max())
    bound = F16_CLOSED[shape.name, shape.causal, d]
    print(f"{rr.hard_id(shape)} d={d}: max|restatement - mean of half(V)| = {err:.2e} (bound {bound:.1e})")
    assert err <= bound, err


@pytest.mark.parametrize("shape", [s for s in rr.HARD_SHAPES if s.name == "underflow"], ids=_ids)
def test_underflow_and_zero_v_are_exactly_zero(oracle_mod, shape):
    """Every score ~100 log2 units below m0 = 0: l stays under both guards (1e-20, 1e-10) and every reference writes
    0; V = 0 gives 0 whatever the scores."""
    for base2 in (True, False):
        assert not hard_int8(shape, 64, base2)[3].any()
    assert not hard_f16(shape, 64)[3].any()
    c = cr.HARD["underflow"]
    Q, K, V = rr.zero_v_hard_inputs(64, shape.Nq, shape.Nk)
    assert Q.any() and K.any() and not V.any()
    assert not rr.fa_int8(oracle_mod, Q, K, V, c.h * 64, c.h, causal=shape.causal, base2=True)[0].any()
    assert not rr.fa_fp16_lazy(None, Q, K, V, c.h * 64, c.h, causal=shape.causal).any()


@pytest.mark.parametrize("shape", [s for s in rr.HARD_SHAPES if s.name == "nan_int8"], ids=_ids)
def test_nan_inputs_reach_the_q_slice_and_the_reference_is_finite(oracle_mod, shape):
    """One NaN lands in the 32 query rows (the kernel's own in-register Q quantisation must zero it), two each in K
    and V (the pre-pass's); the restatement's output is finite."""
    Q, K, V, out, _, _ = hard_int8(shape, 64)
    assert [int(np.isnan(x).sum()) for x in (Q, K, V)] == [1, 2, 2] and np.isnan(Q[0, 4]).any()
    assert np.isfinite(out).all() and np.isfinite(hard_int8(shape, 64, False)[3]).all()


@pytest.mark.parametrize("d", [32, 64, 128])
def test_rows_before_the_spike_do_not_see_it(oracle_mod, d):
    """(160, 256) causal: the query rows are rows 96..255 of the square problem and keys 160..191 one key tile and
    one quantisation group, so rows 0..63 never visit it and are bit-identical to the inputs without the spike;
    query group 2 (its diagonal) and every later row change."""
    pairs = [(hard_int8(SPIKE_CAUSAL, d, b2)[3], hard_int8(SPIKE_CAUSAL, d, b2, spike=False)[3]) for b2 in (True, False)]
    if d in SPIKE_CAUSAL.f16_d:
        pairs.append((hard_f16(SPIKE_CAUSAL, d)[3], hard_f16(SPIKE_CAUSAL, d, spike=False)[3]))
    for spike, plain in pairs:
        assert np.array_equal(spike[:, :64], plain[:, :64])
        assert (spike[:, 64:] != plain[:, 64:]).any(axis=-1).all()


@pytest.mark.parametrize("shape,d", rr.HARD_INT8, ids=_ids)
def test_base2_vs_nats_on_the_hard_shapes_is_recorded(oracle_mod, shape, d):
    """Not asserted, as in DESIGN.md 10.3: at 50..200 log2 units the two statements of the score differ by ~1e-5 in
    the exponent, which can flip a Pi (measured 0 to 0.52 unit here).  Both stay finite."""
    _, _, _, two, pe, _ = hard_int8(shape, d, True)
    nats = hard_int8(shape, d, False)[3]
    apart = cr.flip_units(np.abs(two.astype(np.float64) - nats), pe)
    print(f"{rr.hard_id(shape)} d={d}: base2 vs nats {apart:.2f} one-flip units")
    assert np.isfinite(two).all() and np.isfinite(nats).all()


# ---- the tests can fail: a re-anchor / rebase that does not rescale l, or O -------------------------------------
# a quarter of the smallest distance measured over d on each spike_tile shape.  int8, one-flip units (GPU bound 2):
# stale_l 364..618 on both shapes, stale_o 1277..1681.  fp16, multiples of the GPU bound 2^-10 max|V|: causal stale_l
# 657..737 and stale_o 9283..10201; non-causal (every row carries four tiles of ordinary weight into the spike, none
# a diagonal's handful) 104..129 and 289..326.
INT8_STALE_UNITS = {"stale_l": 364 / 4, "stale_o": 1277 / 4}
F16_STALE_BOUNDS = {(True, "stale_l"): 657 / 4, (True, "stale_o"): 9283 / 4, (False, "stale_l"): 104 / 4,
                    (False, "stale_o"): 288 / 4}


@pytest.mark.parametrize("mutant", cr.RESCALE_MUTANTS)
@pytest.mark.parametrize("d", [32, 64, 128])
@pytest.mark.parametrize("shape", [SPIKE_CAUSAL, SPIKE_FULL], ids=_ids)
def test_int8_rescale_mutants_are_far_outside_the_gpu_bound_on_spike_tile(oracle_mod, shape, d, mutant):
    """The group re-anchors on the spike's tile with O and l of the earlier tiles in hand.  Without `l_run *= f`
    (`o *= f`) they reach the new anchor 2^49..2^98 times too heavy."""
    _, _, _, ref, pe, rise = hard_int8(shape, d)
    bad = hard_int8(shape, d, True, mutant)[3]
    units = cr.flip_units(np.abs(bad.astype(np.float64) - ref), pe)
    print(f"{rr.hard_id(shape)} d={d} {mutant}: {units:.0f} one-flip units from the correct re-anchor (GPU bound 2)")
    assert rise.anchored.any() and units >= INT8_STALE_UNITS[mutant], units
    if shape.causal:  # rows that never meet the spike never re-anchor: untouched
        assert np.array_equal(bad[:, :64], ref[:, :64])


@pytest.mark.parametrize("mutant", cr.RESCALE_MUTANTS)
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("shape", [SPIKE_CAUSAL, SPIKE_FULL], ids=_ids)
def test_fp16_rescale_mutants_are_far_outside_the_gpu_bound_on_spike_tile(shape, d, mutant):
    _, _, V, ref, rebased, _ = hard_f16(shape, d)
    bad = hard_f16(shape, d, mutant)[3]
    tol = 2.0 ** -10 * float(np.abs(V).max())
    err = float(np.abs(bad - ref).max())
    print(f"{rr.hard_id(shape)} d={d} {mutant}: {err / tol:.0f} x the GPU bound")
    assert rebased > 0 and err >= F16_STALE_BOUNDS[shape.causal, mutant] * tol, (err, tol)


@pytest.mark.parametrize("mutant", cr.RESCALE_MUTANTS)
@pytest.mark.parametrize("shape", [CONST_CAUSAL, CONST_FULL], ids=_ids)
def test_const_does_not_move_under_the_rescale_mutants(oracle_mod, shape, mutant):
    """`const` re-anchors / rebases every group, but only on tile 0, where O = l = 0: a missing rescale multiplies
    zeros.  It is here for the overflow a missing RE-ANCHOR would cause (scores 100..200 log2 units above m0), and
    cannot stand in for `spike_tile`: every mutant output is bit-identical to the correct one."""
    for d in shape.int8_d:
        ref, rise = hard_int8(shape, d)[3], hard_int8(shape, d)[5]
        assert (rise.anchored == 1).all() and np.array_equal(hard_int8(shape, d, True, mutant)[3], ref)
    for d in shape.f16_d:
        assert hard_f16(shape, d)[4] > 0 and np.array_equal(hard_f16(shape, d, mutant)[3], hard_f16(shape, d)[3])


def test_ramp_d32_takes_no_reanchor_and_no_mutant_moves_it(oracle_mod):
    """Recorded so that nobody counts on it: `ramp` at d = 32 climbs 34 log2 units in all, the int8 re-anchor never
    fires and both mutants are the correct run.  From d = 64 on it does re-anchor on the accumulated distance, and a
    stale l is 261..334 units out (a stale O, carried 2^48 too heavy through ten more tiles, astronomically)."""
    for shape in (shape_of("ramp", 64, 512, True), shape_of("ramp", 32, 512, False)):
        for mutant in cr.RESCALE_MUTANTS:
            assert np.array_equal(hard_int8(shape, 32, True, mutant)[3], hard_int8(shape, 32)[3])
        for d in (64, 128):
            _, _, _, ref, pe, _ = hard_int8(shape, d)
            units = cr.flip_units(np.abs(hard_int8(shape, d, True, "stale_l")[3].astype(np.float64) - ref), pe)
            print(f"{rr.hard_id(shape)} d={d} stale_l: {units:.0f} one-flip units")
            assert units >= 261 / 4
