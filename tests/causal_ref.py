"""Numpy restatement of the int8 oracle with a `causal` switch, and float64 masked attention.

Helper of tests/test_causal_cpu.py and tests/test_gpu_causal.py (not a test).  oracle/qmha_oracle.c
(fa_int8_item, lines 333-398) is the project's statement of fa_tc_int8_b's intended algorithm and has no
mask; this file restates it step by step in float32 numpy -- the bytes and scales come from
oracle.quantize_heads -- and adds the causal contract of DESIGN.md 10:
  * query group g visits key tiles t = 0..g only;
  * on the diagonal tile t == g a score with j > r is -inf before the row maximum is formed: no part in
    the row max, p = 0 exactly, Pi = 0, nothing in the row sum or in the P-tile absmax.
With causal=False it is the oracle (tests/test_causal_cpu.py holds it to oracle.fa_int8).

Beside O it returns, per row, the ONE-FLIP UNIT u_r: the most one Pi changing by 1 can move an element of
that row.  A flip on tile t moves O[r][d] by |Vi| sP_t sV_t <= 127 sP_t sV_t; that amount is carried
through the later alpha rescales exactly like O, and the output divides by l_r:
    U_r <- max(alpha U_r, 127 sP_t sV_t) per tile,   u_r = U_r / l_r.
The GPU's exp2 and the oracle's expf differ in the last ulp, which can move p / sP across a .5 rounding
boundary; the GPU tests allow two such flips per row, 2 u_r + 5e-5.
"""
import numpy as np

GROUP = 32
_IDX = np.arange(GROUP)


def _xor_tree_sum32(v):
    """The oracle's xor_tree_sum32 over the last axis (shift 16, 8, 4, 2, 1), float32."""
    v = v.astype(np.float32, copy=True)
    for shift in (16, 8, 4, 2, 1):
        v = (v + v[..., _IDX ^ shift]).astype(np.float32)
    return v[..., 0]


def _fma32(a, b, c):
    """fmaf(a, b, c) for float32 arrays: the product of two float32 is exact in float64."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def _quantize_tile(p):
    """oracle_quantize_block on a 32x32 tile of p: (Pi as float32 integers, sP)."""
    f = np.float32
    amax = max(abs(f(p.max())), abs(f(p.min())))
    sc = max(f(f(amax) / f(127.0)), f(1e-8))
    inv = f(1.0) / f(sc)
    q = np.rint((p * inv).astype(f))
    return np.clip(q, -128, 127).astype(f), f(sc)


def fa_int8(oracle, Q, K, V, d_model, h, causal=False):
    """fa_tc_int8_b's intended per-block algorithm; returns (O like Q, u [B, N, h] one-flip units)."""
    f = np.float32
    Q, K, V = (np.ascontiguousarray(x, dtype=f) for x in (Q, K, V))
    squeeze = Q.ndim == 2
    if squeeze:
        Q, K, V = Q[None], K[None], V[None]
    B, N, _ = Q.shape
    d, G = d_model // h, N // GROUP
    (Qi, sQ), (Ki, sK), (Vi, sV) = (oracle.quantize_heads(x, d_model, h) for x in (Q, K, V))
    inv_sqrt_d = f(1.0) / np.sqrt(f(d))
    out = np.zeros_like(Q)
    unit = np.zeros((B, N, h), f)
    future = _IDX[None, :] > _IDX[:, None]  # [r][j]: j > r
    for b in range(B):
        for k in range(h):
            Kf, Vf = Ki[b, k].astype(f), Vi[b, k].astype(f)
            for g in range(G):
                Qg = Qi[b, k, g * GROUP:(g + 1) * GROUP].astype(f)
                O = np.zeros((GROUP, d), f)
                l = np.zeros(GROUP, f)
                m_prev = np.zeros(GROUP, f)  # m0 = 0
                U = np.zeros(GROUP, f)
                for t in range(g + 1 if causal else G):
                    Kt, Vt = Kf[t * GROUP:(t + 1) * GROUP], Vf[t * GROUP:(t + 1) * GROUP]
                    acc = (Qg @ Kt.T).astype(f)  # exact: |acc| <= 127^2 d < 2^24
                    s = ((acc * sQ[b, k, g]).astype(f) * sK[b, k, t]).astype(f)
                    s = (s * inv_sqrt_d).astype(f)
                    if causal and t == g:
                        s = np.where(future, f(-np.inf), s)
                    m_new = np.maximum(m_prev, s.max(axis=1)).astype(f)
                    p = np.exp((s - m_new[:, None]).astype(f)).astype(f)
                    sum_new = _xor_tree_sum32(p)
                    alpha = np.exp((m_prev - m_new).astype(f)).astype(f)
                    l = _fma32(alpha, l, sum_new)
                    O = (O * alpha[:, None]).astype(f)
                    m_prev = m_new
                    Pi, sP = _quantize_tile(p)
                    T = (Pi @ Vt).astype(f)  # exact: |T| <= 32 * 127 * 128 < 2^24
                    ts = (T * sP).astype(f)
                    O = _fma32(ts, np.broadcast_to(sV[b, k, t], ts.shape), O)
                    U = np.maximum((U * alpha).astype(f), f(127.0) * sP * sV[b, k, t]).astype(f)
                ok = l > f(1e-20)
                lsafe = np.where(ok, l, f(1.0))
                rows = slice(g * GROUP, (g + 1) * GROUP)
                out[b, rows, k * d:(k + 1) * d] = np.where(ok[:, None], (O / lsafe[:, None]).astype(f), f(0.0))
                unit[b, rows, k] = np.where(ok, U / lsafe, f(0.0))
    if squeeze:
        return out[0], unit[0]
    return out, unit


def per_element(unit, d):
    """[.., N, h] one-flip units -> [.., N, h*d], the layout of O."""
    return np.repeat(unit, d, axis=-1)


def attention_f64(Q, K, V, d_model, h, causal=False):
    """float64 softmax(Q K^T / sqrt(d)) V per head; causal: row r attends keys j <= r."""
    Q, K, V = (np.asarray(x, dtype=np.float64) for x in (Q, K, V))
    squeeze = Q.ndim == 2
    if squeeze:
        Q, K, V = Q[None], K[None], V[None]
    B, N, _ = Q.shape
    d = d_model // h
    q, k, v = (x.reshape(B, N, h, d).transpose(0, 2, 1, 3) for x in (Q, K, V))
    s = q @ k.transpose(0, 1, 3, 2) / np.sqrt(d)
    if causal:
        s = np.where(np.arange(N)[None, :] > np.arange(N)[:, None], -np.inf, s)
    s -= s.max(-1, keepdims=True)
    p = np.exp(s)
    p /= p.sum(-1, keepdims=True)
    o = (p @ v).transpose(0, 2, 1, 3).reshape(B, N, d_model)
    return o[0] if squeeze else o


# The shapes of tests/test_gpu_causal.py: (N, d_model, h, B, distribution, seed).
CASES = [
    (32, 64, 2, 1, "normal", 101),     # only the diagonal tile; d = 32
    (64, 128, 2, 1, "uniform", 102),
    (96, 64, 1, 1, "normal", 103),     # partly filled workgroup, odd tile count
    (160, 256, 2, 2, "uniform", 104),  # second workgroup with one active wave; d = 128
    (256, 128, 2, 1, "normal", 105),
    (288, 128, 2, 1, "uniform", 106),  # third workgroup of 4-wave groups
    (544, 64, 1, 1, "normal", 107),
    (1024, 128, 2, 2, "normal", 108),  # a long loop
]
# int8 only: more of head size 32 (fa_tc_v1a has no causal d = 32)
CASES_INT8_D32 = [
    (288, 64, 2, 1, "uniform", 109),
    (96, 32, 1, 2, "normal", 110),
]
# fp16 only: the single diagonal tile at a head size fa_tc_v1a is built for
CASES_F16_EXTRA = [
    (32, 128, 2, 1, "normal", 111),
]


def inputs(N, d_model, B, dist, seed):
    rng = np.random.default_rng(seed)
    shape = (B, N, d_model)
    if dist == "normal":
        return [(rng.standard_normal(shape) * 0.5).astype(np.float32) for _ in range(3)]
    return [rng.random(shape, dtype=np.float32) for _ in range(3)]
