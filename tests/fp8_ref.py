"""The fa_tc_fp8 contract (include/launchers.h) restated in numpy: the e4m3 encoding of a cached element,
the layout of a 32-row group's V^T block, and the tile-ordered online softmax with the biased, e4m3-rounded P."""
import numpy as np
import torch

LOG2E = 1.4426950408889634


def encode(x, scale):
    """e4m3_rne(clamp(x / scale, -448, 448)) as bytes; the division and the clamp in fp32."""
    y = np.clip(np.asarray(x, np.float32) / np.float32(scale), np.float32(-448), np.float32(448))
    return torch.from_numpy(np.ascontiguousarray(y)).to(torch.float8_e4m3fn).view(torch.uint8).numpy()


def decode(b):
    return torch.from_numpy(np.ascontiguousarray(b)).view(torch.float8_e4m3fn).to(torch.float32).numpy()


def vt_offset(d, kv):
    """Byte of element (d, kv) in a group's [32 * D]-byte V^T block (fp8_vt_offset, qmha_kernels.hpp)."""
    slot = 16 * (kv >> 4) + 8 * ((kv >> 2) & 1) + (kv & 3) + 4 * ((kv >> 3) & 1)
    return ((d >> 5) * 16 + (d & 15)) * 64 + (slot >> 3) * 16 + ((d >> 4) & 1) * 8 + (slot & 7)


def cache_arrays(K, V, L, k_scale, v_scale):
    """The K and V^T bytes of one K/V head slice holding rows [0, L) of K, V [L, D], zero-padded to ceil32(L)."""
    D, Lp = K.shape[1], -(-L // 32) * 32
    k8, v8 = (np.zeros((Lp, D), np.uint8) for _ in range(2))
    k8[:L], v8[:L] = encode(K[:L], k_scale), encode(V[:L], v_scale)
    vt = np.zeros(Lp * D, np.uint8)
    kv, d = np.meshgrid(np.arange(32), np.arange(D), indexing="ij")
    for g in range(Lp // 32):
        vt[g * 32 * D + vt_offset(d, kv)] = v8[32 * g:32 * g + 32]
    return k8, vt, v8


def attend(q8, k8, v8, L, scales, dtype=np.float64, causal=True):
    """One head: decoded e4m3 Q [Nq, D] (causal: bottom-right aligned; else every row sees all L keys) against the decoded
    cache rows K, V [ceil32(L), D].
    Key tiles of 32 in order; m the true running maximum, p = e4m3(exp2(s - m + 8)) for P@V, l from the unrounded p.
    Returns O, the final l per row, and the largest |v| of the whole slice (the one-flip unit's terms)."""
    q_scale, k_scale, v_scale = scales
    Nq, D = q8.shape
    q8, k8, v8 = (a.astype(dtype) for a in (q8, k8, v8))
    c = dtype(np.float32(q_scale) * np.float32(k_scale) * np.float32(np.float32(1.0 / np.sqrt(np.float32(D))) * np.float32(LOG2E)))
    m, l, o = np.full(Nq, -np.inf, dtype), np.zeros(Nq, dtype), np.zeros((Nq, D), dtype)
    last = np.arange(Nq) + L - Nq if causal else np.full(Nq, L - 1)  # the last key a row sees
    for t in range(0, int(last.max()) + 1, 32):
        s = (q8 @ k8[t:t + 32].T) * c
        s[np.arange(t, t + 32)[None, :] > last[:, None]] = -np.inf
        live = last >= t  # rows whose sweep has ended keep their state
        m_new = np.where(live, np.maximum(m, s.max(axis=1)), m)
        p = np.where(live[:, None], np.exp2(s - m_new[:, None] + dtype(8)), 0).astype(dtype)
        alpha = np.where(np.isfinite(m), np.exp2(m - m_new), 0).astype(dtype)
        l = l * alpha + p.sum(axis=1)
        o = o * alpha[:, None] + decode(encode(p, 1.0)).astype(dtype) @ v8[t:t + 32]
        m = m_new
    return dtype(v_scale) * o / l[:, None], l, np.abs(v8).max() * v_scale
