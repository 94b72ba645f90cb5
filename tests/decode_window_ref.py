"""The windowed decode call of an fp8 cache, with attention sinks (include/launchers.h) restated in numpy on
tests/fp8_ref.py and tests/decode_ref.py: the first tile t0 of a sequence's sweep, the chunks behind it and their two parity
streams with both mask edges, which (row, chunk) partials exist (NaN elsewhere) and which of them are empty, the one-launch
form of a single chunk, the combine of several, and the sink term."""
import numpy as np

from tests import fp8_ref
from tests.decode_ref import layout, views  # noqa: F401 -- the scratch is the decode call's at NCw chunks

EMPTY_M = float(np.float32(-1e30))  # the maximum of a partial that holds no key its row sees: finite, weight 0


def chunks(cap, nq, window, chunk_rows):
    """NCw: a sweep starts at row 64 floor(lo / 64), lo = max(0, L - S), S = nq + window - 1, and ends at row L - 1: L rows
    where L <= S, else S + (L - S) mod 64 <= S + 63 -- at most min(cap, nq + window + 62) rows, whatever L is."""
    tiles = -(-min(cap, nq + window + 62) // 32)
    return -(-tiles // (chunk_rows // 32))


def first_tile(L, nq, window):
    return max(0, L - nq - window + 1) // 64 * 2


def stream(q8, k8, v8, tiles, lim, lo, c):
    """fp8_ref.attend's online softmax of one head over `tiles` (ascending) from the zero state: column r sees key j iff
    lo[r] < j <= lim[r].  A column with no visible key in a tile keeps its state."""
    nq, D = q8.shape
    m, l, o = np.full(nq, -np.inf), np.zeros(nq), np.zeros((nq, D))
    for t in tiles:
        j = np.arange(32 * t, 32 * t + 32)[None, :]
        s = (q8 @ k8[32 * t:32 * t + 32].T) * c
        s[(j > lim[:, None]) | (j <= lo[:, None])] = -np.inf
        live = np.isfinite(s).any(axis=1)
        m_new = np.where(live, np.maximum(m, s.max(axis=1)), m)
        p = np.where(live[:, None], np.exp2(s - np.where(live, m_new, 0)[:, None] + 8.0), 0.0)
        alpha = np.where(np.isfinite(m), np.exp2(m - np.where(np.isfinite(m_new), m_new, 0)), 0.0)
        l, o, m = l * alpha + p.sum(axis=1), o * alpha[:, None] + fp8_ref.decode(fp8_ref.encode(p, 1.0)).astype(np.float64) @ v8[32 * t:32 * t + 32], m_new
    return m, l, o


def sink_term(sink, M):
    """2^(sink log2(e) - M + 8) with the exponent clamped at 120: the 2^8 is the bias l carries."""
    return np.exp2(np.minimum(sink * fp8_ref.LOG2E - M + 8.0, 120.0))


def decode_window(Q, K, V, lens, h, hk, scales, chunk_rows, cap, window, sinks=None):
    """Q [B, nq, h d], K, V [B, cap, hk d] (fp32, raw), sinks [h] or None.  Returns O [B, nq, h d], the scratch (Oc, m, l) with
    NaN where nothing is written (all of it in the one-launch form), Ltot [B, nq, h] with the sink term in it and max|v| of the
    swept rows per (b, head) [B, h] -- float64.  An invalid sequence: zeros, an untouched scratch."""
    (B, nq, _), d, C, G = Q.shape, Q.shape[2] // h, chunk_rows // 32, h // hk
    NC = chunks(cap, nq, window, chunk_rows)
    c = float(np.float32(scales[0]) * np.float32(scales[1]) * np.float32(np.float32(1.0 / np.sqrt(np.float32(d))) * np.float32(fp8_ref.LOG2E)))
    O, Ltot, vmax = np.zeros(Q.shape), np.ones((B, nq, h)), np.ones((B, h))
    Oc, pm, pl = np.full((B, NC, nq, h * d), np.nan), np.full((B, NC, nq, h), np.nan), np.full((B, NC, nq, h), np.nan)
    for b, L in enumerate(lens):
        if not nq <= L <= cap:
            continue
        lim, last, t0 = L - nq + np.arange(nq), (L - 1) // 32, first_tile(L, nq, window)
        assert (last - t0) // C < NC
        for k in range(h):
            kh, qs = k // G, slice(k * d, (k + 1) * d)
            k8, _, v8 = fp8_ref.cache_arrays(K[b][:L, kh * d:(kh + 1) * d], V[b][:L, kh * d:(kh + 1) * d], L, scales[1], scales[2])
            q8, k8, v8 = (fp8_ref.decode(a).astype(np.float64) for a in (fp8_ref.encode(Q[b][:, qs], scales[0]), k8, v8))
            vmax[b, k] = np.abs(v8[32 * t0:]).max() * scales[2]
            for ch in range((last - t0) // C + 1):
                tiles = range(t0 + ch * C, min(t0 + ch * C + C - 1, last) + 1)
                (m0, l0, o0), (m1, l1, o1) = (stream(q8, k8, v8, [t for t in tiles if t % 2 == par], lim, lim - window, c) for par in (0, 1))
                M = np.maximum(m0, m1)
                w0, w1 = (np.where(np.isfinite(m), np.exp2(m - np.where(np.isfinite(M), M, 0)), 0.0) for m in (m0, m1))
                l, o = w0 * l0 + w1 * l1, scales[2] * (w0[:, None] * o0 + w1[:, None] * o1)
                if NC == 1:  # the one-launch form: the sink joins the row sum, O is written, the scratch is not
                    Ltot[b, :, k] = l + (0.0 if sinks is None else sink_term(sinks[k], M))
                    O[b][:, qs] = o / Ltot[b, :, k][:, None]
                    continue
                oc = np.where((l > 1e-10)[:, None], o / np.maximum(l, 1e-300)[:, None], 0.0)  # an empty partial: l = 0, Oc = 0
                rows = ch <= (lim // 32 - t0) // C  # the partials that exist
                Oc[b, ch, rows, qs], pm[b, ch, rows, k], pl[b, ch, rows, k] = oc[rows], np.where(np.isfinite(M), M, EMPTY_M)[rows], l[rows]
            for r in range(nq if NC > 1 else 0):  # the combine
                n = (lim[r] // 32 - t0) // C + 1
                M = pm[b, :n, r, k].max()
                a = pl[b, :n, r, k] * np.exp2(pm[b, :n, r, k] - M)
                Ltot[b, r, k] = a.sum() + (0.0 if sinks is None else sink_term(sinks[k], M))
                O[b, r, qs] = (a[:, None] * Oc[b, :n, r, qs]).sum(axis=0) / Ltot[b, r, k] if Ltot[b, r, k] > 1e-10 else 0.0
    return O, (Oc, pm, pl), Ltot, vmax


def exact(Q, K, V, lens, h, hk, window, sinks=None):
    """float64 band-plus-sink attention on the raw inputs (valid sequences)."""
    (B, nq, _), d, out = Q.shape, Q.shape[2] // h, np.zeros(Q.shape)
    for b, L in enumerate(lens):
        e, j = (np.arange(nq) + L - nq)[:, None], np.arange(L)[None, :]
        for k in range(h):
            kh, qs = k // (h // hk), slice(k * d, (k + 1) * d)
            s = (Q[b][:, qs].astype(np.float64) @ K[b][:L, kh * d:(kh + 1) * d].T.astype(np.float64)) / np.sqrt(d)
            s[(j > e) | (j <= e - window)] = -np.inf
            mx = s.max(axis=1, keepdims=True)
            p = np.exp(s - mx)
            den = p.sum(axis=1, keepdims=True) + (0.0 if sinks is None else np.exp(sinks[k] - mx))
            out[b][:, qs] = (p @ V[b][:L, kh * d:(kh + 1) * d].astype(np.float64)) / den
    return out
