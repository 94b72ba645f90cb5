"""CPU tests behind tests/test_gpu_scale.py: every claim that file makes about its shapes is computed
here from the launch formulas of quantizedmha_amd/csrc/qmha_fa_masked.hip, restated in Python, and asserted -- a test
that silently stops reaching its case is the failure this file exists to catch.  No kernel is launched.

  * the restated formulas (units, masked_nqb, masked_pairs, the two grids, xcd_remap) are found in the source text, so
    a change of the kernels' map fails here and not in a comment;
  * xcd_remap is a bijection on every grid used, and launch index -> (K/V slice, unit block) reaches every pair once;
  * the wide grids of section 1 have a quotient and a remainder over the 8 XCDs, the stated unpaired middle block, the
    stated last unit block with one active wave, and H in {3, 5};
  * the grids of section 3 are at least 1.5 x the resident capacity, taken from profiles/varlen/kres.txt;
  * the inputs of section 2 take neither the int8 re-anchor nor the fp16 rebase (the block is about accumulation over
    128 tiles), and both restatements sit within 4 x their measured distance to float64 there.
The shapes, seeds and input builders live here and are imported by tests/test_gpu_scale.py.
"""
import collections
import functools
import os
import re

import numpy as np
import pytest

from tests import causal_ref as cr
from tests import rect_ref as rr
from tests.gpu_support import F16, INT8

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GROUP, WAVES, STAGE, XCDS = 32, 4, 2, 8  # QMHA_GROUP, kWaves, kSG, the XCDs xcd_remap deals over


# ---- qmha_fa_masked.hip's launch map, restated ------------------------------------------------------------------------
def units(Nq, G=1):
    """SquareCausal / Rect: N / 32 query groups; Grouped / Varlen: G of them per K/V slice."""
    return G * (Nq // GROUP)


def masked_nqb(u):
    return (u + WAVES - 1) // WAVES


def masked_pairs(nqb):
    return (nqb + 1) // 2


def grid(variant, B, h_kv, u):
    """int8: mirrored unit-block pairs; fp16: one unit block per workgroup."""
    nqb = masked_nqb(u)
    return B * h_kv * (masked_pairs(nqb) if variant == INT8 else nqb)


def xcd_remap(orig, nwg):
    q, r = nwg // XCDS, nwg % XCDS
    xcd, slot = orig % XCDS, orig // XCDS
    return (xcd * (q + 1) if xcd < r else r * (q + 1) + (xcd - r) * q) + slot


def blocks_of(variant, launch_index, nwg, nqb):
    """(K/V slice bh, the unit blocks that workgroup runs): masked_wg's pair or masked_wg_single's one block."""
    wg = xcd_remap(launch_index, nwg)
    if variant == INT8:
        bh, pi = divmod(wg, masked_pairs(nqb))
        return bh, sorted({nqb - 1 - pi, pi})
    bh, r = divmod(wg, nqb)
    return bh, [nqb - 1 - r]


def launch_indices(variant, nwg, nqb, bh):
    return [i for i in range(nwg) if blocks_of(variant, i, nwg, nqb)[0] == bh]


# ---- section 1: the wide calls ----------------------------------------------------------------------------------------
# h_kv == h: a multi-head call (G = 1).  Nk of the varlen shape is the cache's capacity.
Wide = collections.namedtuple("Wide", "B h h_kv Nq Nk int8_grid f16_grid")
WIDE = {
    "square": Wide(3, 5, 5, 640, 640, 45, 75),
    "rect": Wide(3, 5, 5, 416, 640, 30, 60),
    "grouped": Wide(3, 9, 3, 160, 288, 18, 36),
    "varlen": Wide(7, 6, 3, 96, 288, 21, 42),
}
VARLEN_LENS = [288, 96, 0, 192, 100, 288, 128]
VARLEN_POS, VARLEN_N = [0, 64, -32, 128, 48, 160, 224], 64
ANCHOR_SLICES = [(0, 0), (2, 4)]  # (b, k) of the square and rect wide calls held to the restatements at d = 64


def wide_inputs(name, d):
    """Q [B, Nq, h d], K and V [B, Nk, h_kv d], rect_ref.inputs' N(0, 0.25)."""
    w = WIDE[name]
    seed = 8100 + 7 * sorted(WIDE).index(name) + d
    Q = rr.inputs(w.Nq, w.Nk, w.h * d, w.B, "normal", seed)[0]
    _, K, V = rr.inputs(w.Nq, w.Nk, w.h_kv * d, w.B, "normal", seed + 1)
    return Q, K, V


def varlen_valid(L, Nq, cap, causal):
    """Varlen::valid"""
    return L % GROUP == 0 and L <= cap and L >= (Nq if causal else GROUP)


# ---- section 2: 128 key tiles -----------------------------------------------------------------------------------------
LONG_NK, LONG_H = 4096, 2
# (name, Nq, causal); the Nq = 32 queries are the last 32 rows of the Nq = 256 ones, so one causal restatement at
# Nq = 256 answers both causal calls (query groups are independent of each other)
LONG_CALLS = [("causal256", 256, True), ("causal32", 32, True), ("full32", 32, False)]
LONG_VARLEN = ([2080, 4096], 4128)  # lens, cap: 65 tiles (odd, a partial last stage far into the loop) and 128 of 129
# measured distance of the restatements to float64 at these shapes, asserted at 4 x
LONG_INT8_TO_F64, LONG_F16_TO_F64 = 3.0e-4, 1.1e-5


@functools.lru_cache(maxsize=None)
def long_inputs(d, dist):
    """Q [1, 256, 2 d], K and V [1, 4096, 2 d] (rect_ref.inputs); read-only."""
    t = rr.inputs(256, LONG_NK, LONG_H * d, 1, dist, 9100 + d + (1 if dist == "uniform" else 0))
    for x in t:
        x.setflags(write=False)
    return t


def long_q(Q, Nq):
    return np.ascontiguousarray(Q[:, Q.shape[1] - Nq:])


def head_cols(X, k, d):
    return np.ascontiguousarray(X[..., k * d:(k + 1) * d])


@functools.lru_cache(maxsize=None)
def long_int8_reference(d, dist, causal, heads=LONG_H):
    """(O, per-element one-flip unit, float64) of the Nq = 256 causal / Nq = 32 unmasked call over the first `heads`
    heads; asserts that no query group re-anchored.  Computed once per process."""
    from oracle import oracle
    Q, K, V = (head_cols(x, 0, heads * d) for x in long_inputs(d, dist))
    Q = Q if causal else long_q(Q, 32)
    ref, unit, rise = rr.fa_int8(oracle, Q, K, V, heads * d, heads, causal=causal, base2=True, stats=True)
    assert int(rise.anchored.max()) == 0, "the long inputs are meant to stay off the re-anchor branch"
    return ref, cr.per_element(unit, d), rr.attention_f64(Q, K, V, heads * d, heads, causal)


@functools.lru_cache(maxsize=None)
def long_f16_reference(d, dist, causal):
    """(lazy contract of head 0 [1, Nq, d], float64 of both heads): the restatement costs 4 s (d = 64) to 12 s (d = 128)
    per head at 4096 keys, so it runs on one head; float64 covers both.  Asserts that no row rebased."""
    Q, K, V = long_inputs(d, dist)
    Q = Q if causal else long_q(Q, 32)
    ref, rebased, _ = rr.fa_fp16_lazy(None, *(head_cols(x, 0, d) for x in (Q, K, V)), d, 1, causal=causal, stats=True)
    assert rebased == 0, "the long inputs are meant to stay off the rebase branch"
    return ref, rr.attention_f64(Q, K, V, LONG_H * d, LONG_H, causal)


# ---- section 3: more workgroups than the device holds -------------------------------------------------------------------
Over = collections.namedtuple("Over", "B h Nq Nk")
OVER_SQUARE = Over(16, 16, 2048, 2048)
OVER_RECT = Over(16, 16, 512, 2048)  # 512 / 1024 workgroups: not kept, see test_grids_exceed_resident_capacity
# K/V slices bh = b * 16 + k: the first, the last, and six whose workgroups all have launch indices in the last third
OVER_SLICES = [(0, 0), (15, 15), (1, 6), (3, 9), (5, 15), (9, 7), (13, 12), (15, 14)]
CUS, LDS_PER_CU = 256, 160 * 1024  # MI355X: compute units, LDS bytes per compute unit (4 SIMDs each, a wave per SIMD)


def resident_capacity(variant, d):
    """256 CUs x min(waves per SIMD, LDS per CU / LDS per workgroup), a workgroup being one wave on each SIMD; the
    two figures are read from the kernel-resource listing the project keeps (tools/kres.py's output)."""
    kernel = {INT8: "qmha_fa_int8_varlen_kernel", F16: "qmha_fa_f16_varlen_kernel"}[variant]
    text = open(os.path.join(ROOT, "profiles", "varlen", "kres.txt")).read().split("# the rows")[0]
    m = re.search(rf"{kernel}ILi{d}E\S*\s+vgpr\s+\d+\s+agpr\s+\d+\s+scratch\s+\d+\s+occ\s+(\d+)\s+lds\s+(\d+)", text)
    occ, lds = int(m.group(1)), int(m.group(2))
    return CUS * min(occ, LDS_PER_CU // lds), occ, lds


# ---- section 4 ---------------------------------------------------------------------------------------------------------
# (Nq, Nk, causal), B = 2, h = 2: a partial last stage (Gk = 5 / 3) and waves that skip tiles or sit idle
AFTER_SHAPES = [(96, 160, True), (160, 96, False)]


# =========================================================================================================================
def test_the_restated_formulas_are_the_sources():
    src = "".join(open(os.path.join(ROOT, "quantizedmha_amd", "csrc", n)).read()  # the geometries' header, then the launchers
                  for n in ("qmha_fa_masked.hpp", "qmha_fa_masked.hip"))
    common = open(os.path.join(ROOT, "quantizedmha_amd", "csrc", "qmha_common.hpp")).read()
    for text in ("constexpr int kWaves = 4, kSG = 2;",
                 "constexpr int masked_pairs(int nqb) { return (nqb + 1) / 2; }",
                 "static int masked_nqb(int units) { return (units + kWaves - 1) / kWaves; }",
                 "const dim3 grid(c.B * c.Hkv * masked_pairs(nqb)), block(kWaves * 64);",
                 "const dim3 grid(c.B * c.Hkv * nqb), block(kWaves * 64);",
                 "bh = wg / nqb;", "qb = nqb - 1 - wg % nqb;",
                 "bh = wg / masked_pairs(nqb);", "pi = wg % masked_pairs(nqb);",
                 "__host__ __device__ int units() const { return N / QMHA_GROUP; }",
                 "__host__ __device__ int units() const { return Nq / QMHA_GROUP; }",
                 "__host__ __device__ int units() const { return G * (Nq / QMHA_GROUP); }"):
        assert text in src, text
    for text in ("const int q = nwg / 8, r = nwg % 8;", "const int xcd = orig % 8, slot = orig / 8;",
                 "return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + slot;"):
        assert text in common, text


def all_grids():
    out = []
    for name, w in WIDE.items():
        u = units(w.Nq, w.h // w.h_kv)
        out += [(f"{name}-{v}", v, grid(v, w.B, w.h_kv, u), masked_nqb(u), w.B * w.h_kv) for v in (INT8, F16)]
    for o in (OVER_SQUARE, OVER_RECT):
        u = units(o.Nq)
        out += [(f"over-Nq{o.Nq}-{v}", v, grid(v, o.B, o.h, u), masked_nqb(u), o.B * o.h) for v in (INT8, F16)]
    for name, Nq, _ in LONG_CALLS:
        out += [(f"long-{name}-{v}", v, grid(v, 1, LONG_H, units(Nq)), masked_nqb(units(Nq)), LONG_H) for v in (INT8, F16)]
    return out


@pytest.mark.parametrize("case", all_grids(), ids=lambda c: c[0])
def test_launch_map_is_a_bijection(case):
    """xcd_remap permutes 0 .. nwg - 1, and launch index -> (slice, unit block) reaches every block of every slice once."""
    _, variant, nwg, nqb, slices = case
    assert sorted(xcd_remap(i, nwg) for i in range(nwg)) == list(range(nwg))
    seen = collections.Counter()
    for i in range(nwg):
        bh, blocks = blocks_of(variant, i, nwg, nqb)
        for qb in blocks:
            seen[(bh, qb)] += 1
    assert set(seen) == {(bh, qb) for bh in range(slices) for qb in range(nqb)} and set(seen.values()) == {1}


@pytest.mark.parametrize("name", list(WIDE))
def test_wide_grids_have_a_quotient_and_a_remainder(name):
    w = WIDE[name]
    G = w.h // w.h_kv
    u = units(w.Nq, G)
    nqb = masked_nqb(u)
    assert (grid(INT8, w.B, w.h_kv, u), grid(F16, w.B, w.h_kv, u)) == (w.int8_grid, w.f16_grid)
    for variant, nwg in ((INT8, w.int8_grid), (F16, w.f16_grid)):
        assert nwg % XCDS != 0, (name, variant, nwg)
        if not (name == "grouped" and variant == INT8):
            assert nwg // XCDS >= 2, (name, variant, nwg)
        # wider than anything the masked suites launched with a remainder before (12 workgroups)
        assert nwg > 12
    assert w.h_kv in (3, 5) and w.B >= 3  # bh / H and bh % H with H beyond {1, 2}
    last_block_active = u - (nqb - 1) * WAVES
    if name == "square":
        assert (u, nqb, masked_pairs(nqb)) == (20, 5, 3) and nqb % 2 == 1
        middle = [blocks for i in range(w.int8_grid) for _, blocks in [blocks_of(INT8, i, w.int8_grid, nqb)] if len(blocks) == 1]
        assert middle == [[2]] * (w.B * w.h)  # the unpaired middle block, once per slice
    elif name == "rect":
        assert (u, nqb, last_block_active) == (13, 4, 1)  # 13 groups: the last unit block has one active wave
        assert (w.Nk - w.Nq) // GROUP == 7  # diag_off, odd: the diagonal opens a stage's second tile
    elif name == "grouped":
        assert (G, u, nqb, last_block_active) == (3, 15, 4, 3)  # a unit block mixes query heads and groups
    else:
        assert (G, u, nqb, last_block_active) == (2, 6, 2, 2)
        for causal in (True, False):
            valid = [varlen_valid(L, w.Nq, w.Nk, causal) for L in VARLEN_LENS]
            assert valid == [True, True, False, True, False, True, True]
        n_ok = [p >= 0 and p % GROUP == 0 and p + VARLEN_N <= w.Nk for p in VARLEN_POS]
        assert n_ok == [True, True, False, True, False, True, True]
        assert max(VARLEN_LENS) == w.Nk and (w.Nk // GROUP) % STAGE == 1  # a full sequence ends in a partial stage


def test_long_loops_are_128_tiles():
    assert LONG_NK // GROUP == 128
    lens, cap = LONG_VARLEN
    assert [L // GROUP for L in lens] == [65, 128] and cap // GROUP == 129
    assert all(L % GROUP == 0 for L in lens + [cap]) and (lens[0] // GROUP) % STAGE == 1  # odd: a partial last stage
    # causal32 / full32: one workgroup per head with one active wave; causal256: two unit blocks, one int8 pair
    assert [grid(INT8, 1, LONG_H, units(Nq)) for _, Nq, _ in LONG_CALLS] == [2, 2, 2]
    assert [grid(F16, 1, LONG_H, units(Nq)) for _, Nq, _ in LONG_CALLS] == [4, 2, 2]


@pytest.mark.parametrize("variant", [INT8, F16])
def test_grids_exceed_resident_capacity(variant):
    cap, occ, lds = resident_capacity(variant, 64)
    assert (occ, lds, cap) == {INT8: (5, 24576, 1280), F16: (4, 32768, 1024)}[variant]
    o = OVER_SQUARE
    nqb = masked_nqb(units(o.Nq))
    nwg = grid(variant, o.B, o.h, units(o.Nq))
    assert (nqb, masked_pairs(nqb), nwg) == (16, 8, {INT8: 2048, F16: 4096}[variant])
    assert nwg >= 1.5 * cap, (nwg, cap)
    # the rectangular shape (B16 h16 Nq512 Nk2048) does not exceed capacity by that margin in either precision, so
    # tests/test_gpu_scale.py does not run it
    r = grid(variant, OVER_RECT.B, OVER_RECT.h, units(OVER_RECT.Nq))
    assert r == {INT8: 512, F16: 1024}[variant] and r < 1.5 * cap
    # the compared slices: the first, the last, and six whose every workgroup is launched in the last third
    assert OVER_SLICES[:2] == [(0, 0), (o.B - 1, o.h - 1)] and len(set(OVER_SLICES)) == 8
    for b, k in OVER_SLICES[2:]:
        idx = launch_indices(variant, nwg, nqb, b * o.h + k)
        assert len(idx) == nwg // (o.B * o.h) and min(idx) >= 2 * nwg / 3, (b, k, min(idx))


# ---- section 2's references: off the hard branches, and close to float64 ------------------------------------------------
@pytest.mark.parametrize("dist", rr.DISTS)
@pytest.mark.parametrize("causal", [True, False], ids=["causal256", "full32"])
def test_long_int8_restatement_stays_plain_and_near_float64(causal, dist):
    """0 re-anchors (asserted where the reference is built) and within 4 x 3.0e-4 of float64, at d = 64, head 0."""
    ref, unit, exact = long_int8_reference(64, dist, causal, heads=1)
    far = float(np.abs(ref - exact).max())
    print(f"int8 restatement, 4096 keys, {dist}, {'causal' if causal else 'full'}: max|ref - float64| = {far:.2e}, "
          f"largest one-flip unit {float(unit.max()):.2e}")
    assert far <= 4 * LONG_INT8_TO_F64, far


@pytest.mark.parametrize("dist", rr.DISTS)
@pytest.mark.parametrize("causal", [True, False], ids=["causal256", "full32"])
def test_long_fp16_restatement_stays_plain_and_near_float64(causal, dist):
    """0 rebased rows (asserted where the reference is built) and within 4 x 1.1e-5 of float64, at d = 64, head 0."""
    ref, exact = long_f16_reference(64, dist, causal)
    far = float(np.abs(ref - exact[..., :64]).max())
    print(f"fp16 restatement, 4096 keys, {dist}, {'causal' if causal else 'full'}: max|ref - float64| = {far:.2e}")
    assert far <= 4 * LONG_F16_TO_F64, far
