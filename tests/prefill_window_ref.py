"""The windowed prefill call of an fp8 cache, with attention sinks (include/launchers.h) restated in numpy on
tests/fp8_ref.py and tests/decode_window_ref.py: per (sequence, head) one stream over the tiles of the sequence's band with both
mask edges -- rows are independent, because a row with no visible key in a tile keeps its state -- and the sink term last."""
import numpy as np

from tests import decode_window_ref as dwr
from tests import fp8_ref


def prefill_window(Q, K, V, lens, h, hk, scales, cap, window, sinks=None):
    """Q [B, nq, h d], K, V [B, cap, hk d] (fp32, raw), sinks [h] or None.  Returns O [B, nq, h d], Ltot [B, nq, h] with the sink
    term in it and max|v| of the swept rows per (b, head) [B, h] -- float64.  An invalid sequence: zeros."""
    (B, nq, _), d, G = Q.shape, Q.shape[2] // h, h // hk
    c = float(np.float32(scales[0]) * np.float32(scales[1]) * np.float32(np.float32(1.0 / np.sqrt(np.float32(d))) * np.float32(fp8_ref.LOG2E)))
    O, Ltot, vmax = np.zeros(Q.shape), np.ones((B, nq, h)), np.ones((B, h))
    for b, L in enumerate(lens):
        if not nq <= L <= cap:
            continue
        lim, tiles = L - nq + np.arange(nq), range(max(0, L - nq - window + 1) // 32, (L - 1) // 32 + 1)
        for k in range(h):
            kh, qs = k // G, slice(k * d, (k + 1) * d)
            k8, _, v8 = fp8_ref.cache_arrays(K[b][:L, kh * d:(kh + 1) * d], V[b][:L, kh * d:(kh + 1) * d], L, scales[1], scales[2])
            q8, k8, v8 = (fp8_ref.decode(a).astype(np.float64) for a in (fp8_ref.encode(Q[b][:, qs], scales[0]), k8, v8))
            vmax[b, k] = np.abs(v8[32 * tiles[0]:]).max() * scales[2]
            m, l, o = dwr.stream(q8, k8, v8, tiles, lim, lim - window, c)
            Ltot[b, :, k] = l + (0.0 if sinks is None else dwr.sink_term(sinks[k], m))
            O[b][:, qs] = scales[2] * o / Ltot[b, :, k][:, None]
    return O, Ltot, vmax
