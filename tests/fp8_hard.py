"""Hard inputs for the e4m3 K/V cache kernels, numpy only: the e4m3 edge table and its placement, score
families in the style of causal_ref.HARD, the contract of tests/fp8_ref.py, decode_ref.py and decode_window_ref.py restated once
more with reach counters and mutants, the stage arithmetic of a decode chunk, and the comparison both test files call.

The instrumented restatement (`attend`, `decode`) is held to the plain ones bit for bit by tests/test_fp8_hard_cpu.py, so a
counter says what the restatement reaches, never what a kernel does.  `mutant=` makes it subtly wrong on purpose:
  mask_after_max  the running maximum is formed over the hidden keys of a swept tile too
  frozen_max      the maximum stays what the first tile made it, p clipped at 448
  merge_no_w      the two parity streams of a chunk are added without their weights 2^(m_i - M)
  combine_skip    the combine leaves out a chunk whose weight 2^(m_c - M) is below 2^-20
  sink_no_clamp   the sink's exponent is not clamped at 120
and `encode_mutant`: round_away (ties away from zero), no_clamp (a value above 448 becomes the NaN byte)."""
import collections
import functools

import numpy as np

from tests import decode_window_ref as dwr
from tests import fp8_ref

FLIPS = 2.0
UNIT, SCALES = (1.0, 1.0, 1.0), (0.3, 0.7, 1.9)
B, CAP = 3, 224
f32 = np.float32

# ---- the edge table ------------------------------------------------------------------------------------------------------
# byte b < 0x7f: exponent field E = b >> 3, mantissa M = b & 7: M 2^-9 (E = 0) or (8 + M) 2^(E - 10)
MAGS = np.array([(b & 7) * 2.0 ** -9 if b < 8 else (8 + (b & 7)) * 2.0 ** ((b >> 3) - 10) for b in range(0x7F)], f32)


def edge_table(inf=True):
    """float32: the 254 finite e4m3 values, every midpoint of adjacent magnitudes (2^-10 among them) with its fp32 neighbours,
    what the clamp sends to +-448 (nextafter(448), 464, 480, 1e30, inf), +-0.0, the least and the largest fp32 subnormal."""
    mid = ((MAGS[:-1].astype(np.float64) + MAGS[1:]) / 2).astype(f32)  # exact: one more bit
    big = [np.nextafter(f32(448), f32(np.inf)), 464.0, 480.0, 1e30] + ([np.inf] if inf else [])
    sub = [np.nextafter(f32(0), f32(1)), np.nextafter(np.finfo(f32).tiny, f32(0))]
    pos = np.concatenate([MAGS, mid, np.nextafter(mid, f32(np.inf)), np.nextafter(mid, f32(0)), np.array(big + sub, f32)])
    return np.concatenate([pos, -pos])


def place(table, L, d, shift=0):
    """[L, d]: row r is the tiled table rolled by 37 r + shift, so rows r, r + 1 overlap in 27 values and a value lands once
    per len(table) / 37 rows, each time in another (r mod 32, d)."""
    return table[(37 * np.arange(L)[:, None] + np.arange(d)[None, :] + shift) % len(table)]


def encode_mutant(x, scale, mutant):
    y = np.asarray(x, f32) / f32(scale)
    if mutant == "no_clamp":
        return np.where(np.abs(y) > 448, np.uint8(0x7F) | (np.signbit(y) * np.uint8(0x80)).astype(np.uint8), fp8_ref.encode(y, 1.0))
    assert mutant == "round_away"
    a = np.minimum(np.abs(y.astype(np.float64)), 448.0)
    step = np.where(a < 2.0 ** -6, 2.0 ** -9, 2.0 ** (np.floor(np.log2(np.maximum(a, 2.0 ** -6))) - 3))
    return fp8_ref.encode((np.floor(a / step + 0.5) * step * np.where(np.signbit(y), -1.0, 1.0)).astype(f32), 1.0)


# ---- the score families --------------------------------------------------------------------------------------------------
FAMILIES = ("rise", "fall", "spike", "oddmax", "evenmax", "chunkmax", "superdiag", "const", "clamp", "zero_q", "zero_v")


@functools.lru_cache(maxsize=None)
def family(name, d, h, hk, nq, lens, cap=CAP):
    """Q [B, nq, h d], K, V [B, cap, hk d], float32.  Q, K ~ N(1, 0.2) (every score positive, about 11 log2 units at d = 64 and
    16 at d = 128 under SCALES), V ~ N(0, 0.5); a family scales rows of K.  The cache holds all `cap` rows, so a key behind
    lens[b] is a masked key of a swept tile like any other."""
    rng = np.random.default_rng([FAMILIES.index(name) if name in FAMILIES else 99, d, hk, cap])
    K, V = rng.normal(1.0, 0.2, (len(lens), cap, hk * d)), rng.normal(0.0, 0.5, (len(lens), cap, hk * d))
    Q = np.random.default_rng([7, d, h, nq]).normal(1.0, 0.2, (len(lens), nq, h * d))
    j = np.arange(cap)
    ramp, tile = (4.0 * j / (cap - 1))[None, :, None], (j // 32)[None, :, None]
    if name == "rise":  # the maximum rises on every tile
        K = K * ramp
    elif name == "fall":  # the maximum is the first tile's; later p fall through e4m3's subnormals to zero
        K = K * ramp[:, ::-1]
    elif name == "spike":  # tile 5 about 150 log2 units above tiles 0 .. 4, tile 6 as much above tile 5
        Q, K[:, 160:192], K[:, 192:224] = Q * 2.5, 6.0, 12.0
    elif name in ("oddmax", "evenmax"):  # the strong keys in the tiles of one parity only
        K = K * np.where(tile % 2 == (name == "oddmax"), 4.0, 0.25)
    elif name == "chunkmax":  # rows 64 .. 127 about 150 log2 units above every other row
        Q, K[:, 64:128] = Q * 2.5, 6.0
    elif name == "superdiag":  # row r's strongest key is its first masked one, L - nq + r + 1
        for b, L in enumerate(lens):
            for r in range(nq):
                if L - nq + r + 1 < cap:
                    K[b, L - nq + r + 1] *= 4.0 + r
    elif name == "const":
        Q[:], K[:] = 3.5, 3.5
    elif name == "clamp":  # about half of the cached bytes are +-448
        Q, K, V = Q * 0.005, K * 320.0, V * 3000.0
    elif name == "zero_q":
        Q[:] = 0.0
    elif name == "zero_v":
        V[:] = 0.0
    else:
        assert name == "normal", name
    return tuple(np.ascontiguousarray(x, f32) for x in (Q, K, V))


# ---- the restatement with counters and mutants ---------------------------------------------------------------------------
def stream(q8, k8, v8, tiles, lim, lo, c, dtype=np.float64, mutant=None, n=None):
    """decode_window_ref.stream (decode_ref.stream at lo = -1; fp8_ref.attend over every tile) in `dtype`; n: a Counter."""
    nq, D = q8.shape
    m, l, o = np.full(nq, -np.inf, dtype), np.zeros(nq, dtype), np.zeros((nq, D), dtype)
    for i, t in enumerate(tiles):
        j = np.arange(32 * t, 32 * t + 32)[None, :]
        raw = (q8 @ k8[32 * t:32 * t + 32].T) * c
        hidden = (j > lim[:, None]) | (j <= lo[:, None])
        s = np.where(hidden, dtype(-np.inf), raw)
        live = np.isfinite(s).any(axis=1)
        top = raw.max(axis=1) if mutant == "mask_after_max" else s.max(axis=1)
        m_new = np.where(live, np.maximum(m, top), m)
        if mutant == "frozen_max":
            m_new = np.where(np.isfinite(m), m, m_new)
        with np.errstate(over="ignore"):
            p = np.where(live[:, None], np.exp2(s - np.where(live, m_new, 0)[:, None] + dtype(8)), 0).astype(dtype)
        if mutant == "frozen_max":
            p = np.minimum(p, dtype(448))
        alpha = np.where(np.isfinite(m), np.exp2(m - np.where(np.isfinite(m_new), m_new, 0)), 0).astype(dtype)
        if n is not None:
            had, seen = np.isfinite(m), ~hidden & live[:, None]
            n["rise_tiles"] += int((had & live & (m_new > m)).any())
            n["still_tiles"] += int(not (live & (m_new > m)).any())
            n["p_subnormal"] += int((seen & (p > 2.0 ** -10) & (p < 2.0 ** -6)).sum())
            n["p_flushed"] += int((seen & (p > 0) & (p <= 2.0 ** -10)).sum())
            n["alpha_underflow"] += int((had & live & (alpha < 2.0 ** -126)).sum())
            n["masked_above"] += int((hidden & live[:, None] & (raw > m_new[:, None])).sum())
        l, o, m = l * alpha + p.sum(axis=1), o * alpha[:, None] + fp8_ref.decode(fp8_ref.encode(p, 1.0)).astype(dtype) @ v8[32 * t:32 * t + 32], m_new
    return m, l, o


def score_scale(scales, d):
    return f32(scales[0]) * f32(scales[1]) * f32(f32(1.0 / np.sqrt(f32(d))) * f32(fp8_ref.LOG2E))


def operands(Qh, Kh, Vh, L, scales, dtype=np.float64, n=None):
    """The decoded e4m3 operands of one head: Q [nq, d], the cache rows K, V [ceil32(L), d] -- with the rows behind L that the
    cache holds (the plain restatements have zeros there; a masked key is -inf either way)."""
    Lp = min(-(-L // 32) * 32, len(Kh))
    k8, _, v8 = fp8_ref.cache_arrays(Kh[:Lp], Vh[:Lp], Lp, scales[1], scales[2])
    if n is not None:
        n["saturated"] += int(((k8 & 0x7F) == 0x7E).sum() + ((v8 & 0x7F) == 0x7E).sum())
        n["bytes"] += 2 * L * k8.shape[1]
    return tuple(fp8_ref.decode(a).astype(dtype) for a in (fp8_ref.encode(Qh, scales[0]), k8, v8))


def attend(Qh, Kh, Vh, L, scales, dtype=np.float64, mutant=None, n=None):
    """fp8_ref.attend (causal) of one head on raw rows: O, l, max|v|."""
    q8, k8, v8 = operands(Qh, Kh, Vh, L, scales, dtype, n)
    lim = L - len(q8) + np.arange(len(q8))
    _, l, o = stream(q8, k8, v8, range((L - 1) // 32 + 1), lim, np.full(len(q8), -1), dtype(score_scale(scales, q8.shape[1])), dtype, mutant, n)
    return dtype(scales[2]) * o / l[:, None], l, np.abs(v8[:L]).max() * scales[2]


def sink_term(sink, M, mutant=None):
    e = sink * fp8_ref.LOG2E - M + 8.0  # in M's precision
    with np.errstate(over="ignore"):
        return np.exp2(e if mutant == "sink_no_clamp" else np.minimum(e, 120.0))


def decode(Q, K, V, lens, h, hk, scales, chunk_rows, cap, window=None, sinks=None, mutant=None, n=None, dtype=np.float64):
    """decode_ref.decode (window None) or decode_window_ref.decode_window: O, (Oc, m, l), Ltot, max|v| of the swept rows.
    The streams, the merge, the combine and the sink term are evaluated in `dtype`; what they give is kept in float64 arrays."""
    (nb, nq, _), d, C, G = Q.shape, Q.shape[2] // h, chunk_rows // 32, h // hk
    NC = -(-cap // chunk_rows) if window is None else dwr.chunks(cap, nq, window, chunk_rows)
    direct, c = window is not None and NC == 1, dtype(score_scale(scales, d))
    O, Ltot, vmax = np.zeros(Q.shape), np.ones((nb, nq, h)), np.ones((nb, h))
    Oc, pm, pl = np.full((nb, NC, nq, h * d), np.nan), np.full((nb, NC, nq, h), np.nan), np.full((nb, NC, nq, h), np.nan)
    for b, L in enumerate(lens):
        if not nq <= L <= cap:
            continue
        lim, last = L - nq + np.arange(nq), (L - 1) // 32
        t0, lo = (0, np.full(nq, -1)) if window is None else (dwr.first_tile(L, nq, window), lim - window)
        for k in range(h):
            kh, qs = k // G, slice(k * d, (k + 1) * d)
            q8, k8, v8 = operands(Q[b][:, qs], K[b][:, kh * d:(kh + 1) * d], V[b][:, kh * d:(kh + 1) * d], L, scales, dtype, n)
            vmax[b, k] = np.abs(v8[32 * t0:L]).max() * scales[2]
            for ch in range((last - t0) // C + 1):
                tiles = range(t0 + ch * C, min(t0 + ch * C + C - 1, last) + 1)
                (m0, l0, o0), (m1, l1, o1) = (stream(q8, k8, v8, [t for t in tiles if t % 2 == par], lim, lo, c, dtype, mutant, n) for par in (0, 1))
                M = np.maximum(m0, m1)
                w0, w1 = (np.where(np.isfinite(m), np.exp2(m - np.where(np.isfinite(M), M, 0)), 0).astype(dtype) for m in (m0, m1))
                if n is not None:
                    n["merge_tiny"] += int(sum((np.isfinite(m) & (w < 2.0 ** -126)).sum() for m, w in ((m0, w0), (m1, w1))))
                    n["merge_small"] += int(sum((np.isfinite(m) & (w < 2.0 ** -24)).sum() for m, w in ((m0, w0), (m1, w1))))
                if mutant == "merge_no_w":
                    w0, w1 = np.isfinite(m0).astype(dtype), np.isfinite(m1).astype(dtype)
                l, o = w0 * l0 + w1 * l1, dtype(scales[2]) * (w0[:, None] * o0 + w1[:, None] * o1)
                if direct:  # one launch: the sink joins the row sum, O is written, the scratch is not
                    lt = l + (dtype(0) if sinks is None else sink_term(sinks[k], M, mutant))
                    Ltot[b, :, k], O[b][:, qs] = lt, o / lt[:, None]
                    continue
                oc = np.where((l > 1e-10)[:, None], o / np.maximum(l, dtype(1e-30))[:, None], 0)
                rows = ch <= (lim // 32 - t0) // C  # the partials that exist
                Oc[b, ch, rows, qs], pm[b, ch, rows, k], pl[b, ch, rows, k] = oc[rows], np.where(np.isfinite(M), M, dwr.EMPTY_M)[rows], l[rows]
                if n is not None:
                    n["partials"] += int(rows.sum())
                    n["empty_partials"] += int((rows & (l == 0)).sum())
            for r in range(0 if direct else nq):  # the combine
                nch = (lim[r] // 32 - t0) // C + 1
                cm, cl, co = (x.astype(dtype) for x in (pm[b, :nch, r, k], pl[b, :nch, r, k], Oc[b, :nch, r, qs]))
                Mx = cm.max()
                wt = np.exp2(cm - Mx)
                if n is not None:
                    n["combine_tiny"] += int((wt < 2.0 ** -126).sum())
                if mutant == "combine_skip":
                    wt = np.where(wt < 2.0 ** -20, 0, wt).astype(dtype)
                a = cl * wt
                lt = a.sum() + (dtype(0) if sinks is None else sink_term(sinks[k], Mx, mutant))
                Ltot[b, r, k], O[b, r, qs] = lt, (a[:, None] * co).sum(axis=0) / lt if lt > 1e-10 else 0.0
    return O, (Oc, pm, pl), Ltot, vmax


def high_sinks(Q, K, V, lens, h, hk, cap):
    """Per head, in natural-log units: 130 log2 units and more above every score of the call (the clamp at 120)."""
    _, (_, pm, _), _, _ = decode(Q, K, V, lens, h, hk, SCALES, 64, cap)
    return ((np.nanmax(pm) + 130.0 + 10.0 * np.arange(h)) / fp8_ref.LOG2E).astype(f32)


def counters():
    return collections.Counter()


# ---- the stages of a decode chunk ----------------------------------------------------------------------------------------
def stages(L, nq, chunk_rows, window=None):
    """Per chunk of a valid sequence's sweep: (t0, stages nst, tiles in the last stage, tiles in the chunk)."""
    C, t0, last = chunk_rows // 32, 0 if window is None else dwr.first_tile(L, nq, window), (L - 1) // 32
    out = []
    for first in range(t0, last + 1, C):
        tiles = min(first + C - 1, last) - first + 1
        out.append((t0, -(-tiles // 2), 2 - tiles % 2, tiles))
    return out


# ---- the comparison ------------------------------------------------------------------------------------------------------
def fp32_term(V, scales):
    """2^-16 max|V|, of what the cache can hold of V: the clamp's 448 v_scale at most."""
    return 2.0 ** -16 * min(float(np.abs(V).max()), 448.0 * scales[2])


def o_bound(vmax, l, d, fp32, flips=FLIPS):
    """FLIPS one-flip units 2^-4 2^8 max|v| / l per element plus the fp32 term: vmax [B, h], l [B, (NC,) nq, h] -> [.., h d]."""
    unit = vmax.reshape((vmax.shape[0],) + (1,) * (l.ndim - 2) + (vmax.shape[1],))
    return np.repeat(flips * 2.0 ** 4 * unit / l, d, axis=-1) + fp32


def compare(label, got, ref, bound):
    """What both test files hold O (or the partials) to: finite and within the bound of the restatement.  Returns the worst
    err / bound."""
    assert np.isfinite(got).all(), (label, "not finite")
    err = np.abs(np.asarray(got, np.float64) - ref)
    worst = float(np.divide(err, bound, out=np.zeros_like(err), where=bound > 0).max()) if err.size else 0.0  # zero_v: 0 <= 0
    assert (err <= bound).all(), (label, worst)
    return worst


def compare_sunk(label, got, want, keys, d, fp32):
    """O of a call whose sinks take nearly all of a row's weight, against the restatement `want`.  The row's keys weigh keys /
    Ltot together (keys: the Ltot of the same call without sinks), so O is that far below max|V| and the fp32 term of the bound
    -- the rounding of a sum whose weights add up to 1 -- shrinks by the same factor; the one-flip units divide by Ltot as
    ever.  Where the restatement's O stands clear of the bound, O is not 0: a sink term that overflowed would give o / inf."""
    O, _, Ltot, vmax = want
    bound = o_bound(vmax, Ltot, d, 0.0) + fp32 * np.repeat(keys / Ltot, d, axis=-1)
    worst, clear = compare(label, got, O, bound), np.abs(O) > 2.0 * bound
    assert clear.any() and (np.asarray(got)[clear] != 0).all(), (label, "O is 0 where the contract's is not")
    return worst


def same_bits(label, got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (label, got.dtype, want.dtype, got.shape, want.shape)
    u = {1: np.uint8, 4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    assert np.array_equal(got.view(u), want.view(u)), (label, int((got.view(u) != want.view(u)).sum()))


def uniform_mean(Q, K, V, lens, h, hk, scales, window=None):
    """`const`: every score of a row is the same, so O is the float64 mean of the decoded V rows the row sees."""
    (nb, nq, _), d, out = Q.shape, Q.shape[2] // h, np.zeros(Q.shape)
    for b, L in enumerate(lens):
        for k in range(h):
            kh = k // (h // hk)
            v8 = fp8_ref.decode(fp8_ref.encode(V[b][:L, kh * d:(kh + 1) * d], scales[2])).astype(np.float64) * scales[2]
            for r in range(nq):
                e = L - nq + r
                out[b, r, k * d:(k + 1) * d] = v8[max(0, e - window + 1) if window else 0:e + 1].mean(axis=0)
    return out


# ---- the cases of tests/test_gpu_fp8_hard.py (tests/test_fp8_hard_cpu.py counts what they reach) ----------------------------
HEADS = [(2, 2, 1), (4, 1, 5), (8, 2, 8)]  # h, h_kv, Nq of the decode calls: W = 1, 20, 32 columns
PREFILL = [(5, (33, 95, 224)), (40, (40, 100, 224))]  # Nq, lengths of attend_tokens / attend_paged
CHUNKS, WINDOWS = (64, 128), (1, 33, 100)
BIG_B, BIG_CAP = 2, 768
BIG_HEADS = [(2, 2, 1), (8, 2, 8), (32, 1, 1)]
BIG_CHUNKS, BIG_PAGES = (192, 256, 320, 768), (64, 128, 192, 384)
BIG_WINDOWS = [(128, 256), (128, 64), (500, 192), (1024, 192)]  # window, chunk_rows: one launch; combine; wide; >= cap


def lens_of(nq, kind):
    return (nq, 65, 224) if kind == "edge" else (33, 95, 193)


def big_lens(nq):
    return [(nq, 449), (257, 768), (193, 705)]


def ramp(h):
    return np.linspace(-2.0, 3.0, h).astype(f32) if h > 1 else np.array([3.0], f32)
