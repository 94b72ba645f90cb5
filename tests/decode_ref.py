"""The decode call of an fp8 cache (include/launchers.h) restated in numpy on tests/fp8_ref.py: per column the
two streams of a chunk by tile parity, their merge, which (row, chunk) partials exist (NaN elsewhere) and the combine."""
import numpy as np

from tests import fp8_ref


def layout(B, NC, nq, h, d):
    """The scratch: float32 offsets of Oc [B, NC, nq, h d], m and l [B, NC, nq, h], and the byte size; each array on 256 bytes."""
    al = lambda x: -(-x // 256) * 256  # noqa: E731
    o, s = 4 * B * NC * nq * h * d, 4 * B * NC * nq * h
    return (0, al(o) // 4, (al(o) + al(s)) // 4), al(o) + 2 * al(s)


def views(scratch, B, NC, nq, h, d):
    """(Oc, m, l) of a float32 view of the scratch bytes."""
    (o, m, l), _ = layout(B, NC, nq, h, d)
    n = B * NC * nq * h
    return scratch[o:o + n * d].reshape(B, NC, nq, h * d), scratch[m:m + n].reshape(B, NC, nq, h), scratch[l:l + n].reshape(B, NC, nq, h)


def stream(q8, k8, v8, tiles, lim, c):
    """fp8_ref.attend's online softmax of one head over `tiles` (ascending) from the zero state: column r sees key j <= lim[r]."""
    nq, D = q8.shape
    m, l, o = np.full(nq, -np.inf), np.zeros(nq), np.zeros((nq, D))
    for t in tiles:
        s = (q8 @ k8[32 * t:32 * t + 32].T) * c
        s[np.arange(32 * t, 32 * t + 32)[None, :] > lim[:, None]] = -np.inf
        live = lim >= 32 * t  # a column with no key in the tile keeps its state
        m_new = np.where(live, np.maximum(m, s.max(axis=1)), m)
        p = np.where(live[:, None], np.exp2(s - np.where(live, m_new, 0)[:, None] + 8.0), 0.0)
        alpha = np.where(np.isfinite(m), np.exp2(m - np.where(np.isfinite(m_new), m_new, 0)), 0.0)
        l, o, m = l * alpha + p.sum(axis=1), o * alpha[:, None] + fp8_ref.decode(fp8_ref.encode(p, 1.0)).astype(np.float64) @ v8[32 * t:32 * t + 32], m_new
    return m, l, o


def decode(Q, K, V, lens, h, hk, scales, chunk_rows, cap):
    """Q [B, nq, h d], K, V [B, cap, hk d] (fp32, raw).  Returns O [B, nq, h d], the scratch (Oc, m, l) with NaN where nothing is
    written, Ltot [B, nq, h] and max|v| per (b, head) [B, h] -- float64.  An invalid sequence: zeros, an untouched scratch."""
    (B, nq, _), d, C, NC, G = Q.shape, Q.shape[2] // h, chunk_rows // 32, -(-cap // chunk_rows), h // hk
    c = float(np.float32(scales[0]) * np.float32(scales[1]) * np.float32(np.float32(1.0 / np.sqrt(np.float32(d))) * np.float32(fp8_ref.LOG2E)))
    O, Ltot, vmax = np.zeros(Q.shape), np.ones((B, nq, h)), np.ones((B, h))
    Oc, pm, pl = np.full((B, NC, nq, h * d), np.nan), np.full((B, NC, nq, h), np.nan), np.full((B, NC, nq, h), np.nan)
    for b, L in enumerate(lens):
        if not nq <= L <= cap:
            continue
        lim, last = L - nq + np.arange(nq), (L - 1) // 32
        for k in range(h):
            kh, qs = k // G, slice(k * d, (k + 1) * d)
            k8, _, v8 = fp8_ref.cache_arrays(K[b][:L, kh * d:(kh + 1) * d], V[b][:L, kh * d:(kh + 1) * d], L, scales[1], scales[2])
            q8, k8, v8 = (fp8_ref.decode(a).astype(np.float64) for a in (fp8_ref.encode(Q[b][:, qs], scales[0]), k8, v8))
            vmax[b, k] = np.abs(v8).max() * scales[2]
            for ch in range(last // C + 1):
                tiles = range(ch * C, min(ch * C + C - 1, last) + 1)
                (m0, l0, o0), (m1, l1, o1) = (stream(q8, k8, v8, [t for t in tiles if t % 2 == par], lim, c) for par in (0, 1))
                M = np.maximum(m0, m1)
                w0, w1 = (np.where(np.isfinite(m), np.exp2(m - np.where(np.isfinite(M), M, 0)), 0.0) for m in (m0, m1))
                l = w0 * l0 + w1 * l1
                oc = np.where((l > 1e-10)[:, None], scales[2] * (w0[:, None] * o0 + w1[:, None] * o1) / np.maximum(l, 1e-300)[:, None], 0.0)
                rows = ch <= lim // 32 // C  # the partials that exist
                Oc[b, ch, rows, qs], pm[b, ch, rows, k], pl[b, ch, rows, k] = oc[rows], M[rows], l[rows]
            for r in range(nq):  # the combine
                n = lim[r] // 32 // C + 1
                a = pl[b, :n, r, k] * np.exp2(pm[b, :n, r, k] - pm[b, :n, r, k].max())
                Ltot[b, r, k] = a.sum()
                O[b, r, qs] = (a[:, None] * Oc[b, :n, r, qs]).sum(axis=0) / a.sum() if a.sum() > 1e-10 else 0.0
    return O, (Oc, pm, pl), Ltot, vmax


def exact(Q, K, V, lens, h, hk):
    """float64 causal attention on the raw inputs (valid sequences)."""
    (B, nq, _), d, out = Q.shape, Q.shape[2] // h, np.zeros(Q.shape)
    for b, L in enumerate(lens):
        for k in range(h):
            kh, qs = k // (h // hk), slice(k * d, (k + 1) * d)
            s = (Q[b][:, qs].astype(np.float64) @ K[b][:L, kh * d:(kh + 1) * d].T.astype(np.float64)) / np.sqrt(d)
            s[np.arange(L)[None, :] > (np.arange(nq) + L - nq)[:, None]] = -np.inf
            p = np.exp(s - s.max(axis=1, keepdims=True))
            out[b][:, qs] = (p @ V[b][:L, kh * d:(kh + 1) * d].astype(np.float64)) / p.sum(axis=1, keepdims=True)
    return out
