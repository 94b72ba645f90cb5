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

Also here: fa_int8's base2 switch (the causal kernel's own score arithmetic) and its Rise record (did the
inputs take the kernel's re-anchor branch?); fa_fp16_lazy, the fp16 kernel's contract (oracle fa_fp16_lazy_item)
restated with the same mask, which counts the rows that rebase; and HARD_CASES, inputs that take those two
branches on and off the diagonal tile and put every row's strongest key just behind the mask.  Both
restatements take a private _mutant= (two wrong masks, two missing rescales) so the CPU tests can show that the
hard cases would catch one.
"""
import collections

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


# Per row [B, N, h].  log2 / diag: the largest rise of the row's running max over ONE tile, and whether that tile was
# t == g.  anchored / anchored_diag: on how many tiles the row's wave took the kernel's re-anchor branch -- any
# of its 32 rows with m_new - anchor > 48, anchor the m of the last such tile (0 at the start) -- and whether one of
# them was t == g.  A one-tile rise above 48 always re-anchors (anchor <= the previous m); a slow climb does too.
Rise = collections.namedtuple("Rise", "log2 diag anchored anchored_diag")
REANCHOR = 48.0


def softmax_scale_log2(d):
    """The host constant of the fused kernels (qmha_kernels.hpp): (1 / sqrtf(d)) * log2 e in float32."""
    f = np.float32
    return f((f(1.0) / np.sqrt(f(d))) * f(1.4426950408889634))


MASK_MUTANTS = ("mask_after_max", "leak_next")
# a re-anchoring group (int8) or a rebasing row (fp16) whose l / whose O keeps the scale it had before the branch
RESCALE_MUTANTS = ("stale_l", "stale_o")
_MUTANTS = (None,) + MASK_MUTANTS + RESCALE_MUTANTS


def _future(mutant):
    """[r][j] mask of the diagonal tile: j > r; the "leak_next" mutant lets key r + 1 through."""
    return _IDX[None, :] > _IDX[:, None] + (1 if mutant == "leak_next" else 0)


def fa_int8(oracle, Q, K, V, d_model, h, causal=False, base2=False, _mutant=None):
    """fa_tc_int8_b's intended per-block algorithm; returns (O like Q, u [B, N, h] one-flip units, Rise).

    base2=False is the C oracle's score arithmetic in nats, exp((acc sQ sK) / sqrt(d) - m).  base2=True is the
    causal kernel's (qmha_fa_masked.hip:247-266): c = (sQ c_log2) sK with the host's c_log2, m_new =
    max(m, mx c), p = exp2(fma(s, c, -m_new)), alpha = exp2(m - m_new); everything else is unchanged.  At scores
    of 50..200 log2 units the two forms differ by ~1e-5 in the exponent, enough to flip a Pi.
    Rise.log2[b, r, k] is the largest rise of row r's running max over one tile in log2 units (the kernel
    re-anchors when m_new - anchor > 48, and anchor <= the previous m), Rise.diag whether that tile was the
    diagonal one.  _mutant (tests only) selects a wrong mask: "mask_after_max" forms the row max over the
    unmasked scores, "leak_next" masks j > r + 1; or a wrong re-anchor: on a tile where the group re-anchors,
    "stale_l" is the kernel without `l_run *= f` and "stale_o" the kernel without `o *= f` -- the kernel holds
    l 2^(m - anchor) and O 2^(m - anchor), so the state that is not rescaled reaches the new anchor as
    2^(m_prev - old anchor) >= 1 times its value where the correct factor is alpha = 2^(m_prev - m_new)."""
    assert _mutant in _MUTANTS
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
    rise_log2 = np.zeros((B, N, h), f)
    rise_diag = np.zeros((B, N, h), bool)
    anchored = np.zeros((B, N, h), np.int64)
    anchored_diag = np.zeros((B, N, h), bool)
    future = _future(_mutant)  # [r][j]: j > r
    c_log2 = softmax_scale_log2(d)
    ex = np.exp2 if base2 else np.exp
    to_log2 = f(1.0) if base2 else f(1.4426950408889634)
    for b in range(B):
        for k in range(h):
            Kf, Vf = Ki[b, k].astype(f), Vi[b, k].astype(f)
            for g in range(G):
                Qg = Qi[b, k, g * GROUP:(g + 1) * GROUP].astype(f)
                O = np.zeros((GROUP, d), f)
                l = np.zeros(GROUP, f)
                m_prev = np.zeros(GROUP, f)  # m0 = 0
                U = np.zeros(GROUP, f)
                rise = np.zeros(GROUP, f)
                on_diag = np.zeros(GROUP, bool)
                anchor = np.zeros(GROUP, f)
                n_anchor, anchor_diag = 0, False
                for t in range(g + 1 if causal else G):
                    Kt, Vt = Kf[t * GROUP:(t + 1) * GROUP], Vf[t * GROUP:(t + 1) * GROUP]
                    acc = (Qg @ Kt.T).astype(f)  # exact: |acc| <= 127^2 d < 2^24
                    diag = causal and t == g
                    if base2:  # the kernel: raw integer scores, one constant, the product inside the fma
                        c = f(f(sQ[b, k, g] * c_log2) * sK[b, k, t])
                        s = acc
                    else:
                        s = ((acc * sQ[b, k, g]).astype(f) * sK[b, k, t]).astype(f)
                        s = (s * inv_sqrt_d).astype(f)
                    unmasked_max = s.max(axis=1)
                    if diag:
                        s = np.where(future, f(-np.inf), s)
                    mx = unmasked_max if diag and _mutant == "mask_after_max" else s.max(axis=1)
                    if base2:
                        m_new = np.maximum(m_prev, (mx * c).astype(f)).astype(f)
                        p = np.exp2(_fma32(s, np.broadcast_to(c, s.shape), -m_new[:, None])).astype(f)
                    else:
                        m_new = np.maximum(m_prev, mx).astype(f)
                        p = np.exp((s - m_new[:, None]).astype(f)).astype(f)
                    up = (m_new - m_prev) * to_log2
                    on_diag = np.where(up > rise, diag, on_diag)
                    rise = np.maximum(rise, up).astype(f)
                    alpha = ex((m_prev - m_new).astype(f)).astype(f)
                    alpha_l = alpha_o = alpha
                    if ((m_new - anchor) * to_log2 > f(REANCHOR)).any():  # wave-uniform (a ballot) in the kernel
                        if _mutant in RESCALE_MUTANTS:
                            stale = ex((m_prev - anchor).astype(f)).astype(f)
                            alpha_l, alpha_o = (stale, alpha) if _mutant == "stale_l" else (alpha, stale)
                        anchor = m_new
                        n_anchor += 1
                        anchor_diag |= bool(diag)
                    sum_new = _xor_tree_sum32(p)
                    l = _fma32(alpha_l, l, sum_new)
                    O = (O * alpha_o[:, None]).astype(f)
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
                rise_log2[b, rows, k] = rise
                rise_diag[b, rows, k] = on_diag
                anchored[b, rows, k] = n_anchor
                anchored_diag[b, rows, k] = anchor_diag
    if squeeze:
        return out[0], unit[0], Rise(rise_log2[0], rise_diag[0], anchored[0], anchored_diag[0])
    return out, unit, Rise(rise_log2, rise_diag, anchored, anchored_diag)


def per_element(unit, d):
    """[.., N, h] one-flip units -> [.., N, h*d], the layout of O."""
    return np.repeat(unit, d, axis=-1)


def flip_units(err, unit_per_element):
    """The worst (err - 5e-5) / u_r: how many one-flip units an output is away, beyond the 5e-5 floor."""
    return float((np.maximum(err - 5e-5, 0.0) / np.maximum(unit_per_element, 1e-30)).max())


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


# ---- the fp16 kernel's own contract, restated with the mask ---------------------------------------------
LAZY_CAP = np.float32(4096.0)  # kLazySumCapC
# key of slot j of lane group (quarter) hh: kap16(j >> 2, 4 hh + (j & 3))
_QUARTER = np.array([[16 * (mm >> 3) + 4 * ((mm >> 2) & 1) + (mm & 3) + 8 * (j >> 2)
                      for j in range(8) for mm in [4 * hh + (j & 3)]] for hh in range(4)])


def _half(x):
    return x.astype(np.float16).astype(np.float32)


def _quarter_sums(p):
    """[R, 32] -> [R, 4]: each lane group's eight keys, summed in the kernel's tree order."""
    q = p[:, _QUARTER]  # [R, 4, 8]
    return ((q[..., 0] + q[..., 1]) + (q[..., 2] + q[..., 3])) + ((q[..., 4] + q[..., 5]) + (q[..., 6] + q[..., 7]))


def fp16_lazy_tol(N):
    """tests/test_gpu_parity.py's bound of the fp16 kernel against its own contract (oracle.fa_fp16_lazy)."""
    return 1e-4 if N <= 256 else 4e-5


def fa_fp16_lazy(oracle, Q, K, V, d_model, h, causal=False, _mutant=None, per_row=False):
    """float32 numpy restatement of oracle/qmha_oracle.c:fa_fp16_lazy_item, quarters form (d = 64, 128), with the
    causal contract of DESIGN.md 10.1; returns (O like Q, rebased (row, tile) pairs, those on a diagonal tile).

    Q, K, V rounded to half; S accumulated by fmaf over d (half x half is exact in float32, so a float32
    multiply-add IS the fma); p = exp2(fma(S, c, -m)) with c = (1 / sqrtf(d)) log2 e against the per-row lazy
    base m (m0 = 0).  When one of a row's four key quarters sums above 2^12 on a tile the row moves to that
    tile's row max, O and l scale by exp2(m_old - m_new) and the tile's p are recomputed.  l is kept per
    quarter; the guard is l > 1e-10.  causal: group g visits tiles 0..g and on the diagonal tile j > r is -inf
    before anything uses the score, so a masked key takes no part in a quarter sum or in the rebase's row
    max.  All groups advance together, tile by tile (`oracle` is unused: the signature mirrors fa_int8).
    _mutant as in fa_int8; here "stale_l" / "stale_o" leave l / O of a rebasing row unscaled (the kernel without
    `l_run[qb] *= alpha` / `o[m][qb] *= alpha`).  per_row=True returns the two counts per row, [B, N, h], instead
    of their totals."""
    assert _mutant in _MUTANTS
    f = np.float32
    Q, K, V = (np.ascontiguousarray(x, dtype=f) for x in (Q, K, V))
    squeeze = Q.ndim == 2
    if squeeze:
        Q, K, V = Q[None], K[None], V[None]
    B, N, _ = Q.shape
    d, G = d_model // h, N // GROUP
    assert d in (64, 128), "quarters form only"
    c = softmax_scale_log2(d)
    future = _future(_mutant)
    out = np.zeros_like(Q)
    rebased = np.zeros((B, N, h), np.int64)
    rebased_diag = np.zeros((B, N, h), np.int64)
    with np.errstate(over="ignore"):  # p overflows to inf before a rebase, as in the kernel
        for b in range(B):
            for k in range(h):
                q, kk, v = (_half(x[b, :, k * d:(k + 1) * d]) for x in (Q, K, V))
                S = np.zeros((N, N), f)
                for e in range(d):
                    S += q[:, e, None] * kk[None, :, e]
                m = np.zeros(N, f)
                l = np.zeros((N, 4), f)
                O = np.zeros((N, d), f)
                for t in range(G):
                    r0 = t * GROUP if causal else 0
                    s = S[r0:, t * GROUP:(t + 1) * GROUP].copy()
                    unmasked_max = s[:GROUP].max(axis=1)
                    if causal:
                        s[:GROUP] = np.where(future, f(-np.inf), s[:GROUP])
                    mx = s.max(axis=1)
                    if causal and _mutant == "mask_after_max":
                        mx[:GROUP] = unmasked_max
                    p = np.exp2(_fma32(s, np.broadcast_to(c, s.shape), -m[r0:, None])).astype(f)
                    ts = _quarter_sums(p)
                    over = (ts > LAZY_CAP).any(axis=1)
                    if over.any():
                        rows = r0 + np.nonzero(over)[0]
                        xm = (mx[over] * c).astype(f)
                        alpha = np.exp2((m[rows] - xm).astype(f)).astype(f)
                        if _mutant != "stale_l":
                            l[rows] *= alpha[:, None]
                        if _mutant != "stale_o":
                            O[rows] *= alpha[:, None]
                        m[rows] = xm
                        p[over] = np.exp2(_fma32(s[over], np.broadcast_to(c, s[over].shape), -xm[:, None])).astype(f)
                        ts[over] = _quarter_sums(p[over])
                        rebased[b, rows, k] += 1
                        if causal:
                            rebased_diag[b, rows[rows < r0 + GROUP], k] += 1
                    ph = _half(p)
                    l[r0:] += ts
                    vt = v[t * GROUP:(t + 1) * GROUP]
                    acc = np.zeros((N - r0, d), f)
                    for j in range(GROUP):
                        acc += ph[:, j, None] * vt[j][None, :]
                    O[r0:] = acc + O[r0:]
                lr = (l[:, 0] + l[:, 1]) + (l[:, 2] + l[:, 3])
                ok = lr > f(1e-10)
                out[b, :, k * d:(k + 1) * d] = np.where(ok[:, None], O / np.where(ok, lr, f(1.0))[:, None], f(0.0))
    if not per_row:
        return (out[0] if squeeze else out), int(rebased.sum()), int(rebased_diag.sum())
    return (out[0], rebased[0], rebased_diag[0]) if squeeze else (out, rebased, rebased_diag)


# ---- hard inputs: the re-anchor (int8) and rebase (fp16) branches, the mask before the max ----------------
def _const(d, h, N, B):
    rng = np.random.default_rng(201)
    Q = np.full((B, N, h * d), 3.5, np.float32)
    return Q, Q.copy(), rng.standard_normal((B, N, h * d)).astype(np.float32)


def _superdiag(d, h, N, B):
    rng = np.random.default_rng(202)
    Q, K = ((rng.standard_normal((B, N, h * d)) * 0.5).astype(np.float32) for _ in range(2))
    K[:, 1:] = 32.0 * Q[:, :-1]  # the strongest key of row r is r + 1, its first masked one
    return Q, K, rng.standard_normal((B, N, h * d)).astype(np.float32)


def _ramp(d, h, N, B):  # tests/test_gpu_parity.py test_growing_scores_reanchor
    rng = np.random.default_rng(7)
    shape = (B, N, h * d)
    Q = (rng.standard_normal(shape) * 0.2 + 1.0).astype(np.float32)
    ramp = np.linspace(0.0, 4.0, N, dtype=np.float32)[None, :, None]
    K = ((rng.standard_normal(shape) * 0.2 + 1.0) * ramp).astype(np.float32)
    return Q, K, rng.standard_normal(shape).astype(np.float32)


SPIKE = slice(160, 192)  # key tile 5


def _spike_tile(d, h, N, B, spike=True):  # test_large_first_tile_and_spike_no_overflow, part (2)
    rng = np.random.default_rng(40 + d)
    shape = (B, N, h * d)
    V = rng.standard_normal(shape).astype(np.float32)
    Q = (rng.standard_normal(shape) * 0.3 + 1.0).astype(np.float32)
    K = (rng.standard_normal(shape) * 0.3).astype(np.float32)
    if spike:
        K[:, SPIKE] = 6.0
    return Q, K, V


def _staircase(d, h, N, B):  # test_lazy_base_staircase with the fp16 cap
    cap = 4096.0
    rng = np.random.default_rng(int(cap) + d)
    shape = (B, N, h * d)
    Q = (0.5 + 0.01 * rng.standard_normal(shape)).astype(np.float32)
    unit = 1.0 / (0.5 * np.sqrt(d) * np.log2(np.e))  # level per log2 unit of score
    hi = np.arange(N // 32) * 0.95 * np.log2(cap) * unit
    level = np.repeat(hi, 32) - 8.0 * unit
    level[0::32] = hi  # keys 0 and 4 lead their tile: on the diagonal tile rows 0..3 see one of them, later rows two
    level[4::32] = hi
    K = (level[None, :, None] + 0.01 * rng.standard_normal(shape)).astype(np.float32)
    return Q, K, rng.standard_normal(shape).astype(np.float32)


def _underflow(d, h, N, B):  # test_underflow_guard_and_zero_v, part (1)
    rng = np.random.default_rng(8)
    shape = (B, N, h * d)
    Q = np.full(shape, 3.0, np.float32)
    K = np.full(shape, -3.0, np.float32) + (rng.standard_normal(shape) * 0.01).astype(np.float32)
    return Q, K, rng.standard_normal(shape).astype(np.float32)


def zero_v_inputs(d, h, N, B):  # test_underflow_guard_and_zero_v, part (2): any finite attention of V = 0 is 0
    rng = np.random.default_rng(9)
    Q, K = (rng.standard_normal((B, N, h * d)).astype(np.float32) for _ in range(2))
    return Q, K, np.zeros((B, N, h * d), np.float32)


def _zero_q(d, h, N, B):  # test_edge_values, part (1)
    rng = np.random.default_rng(99)
    shape = (B, N, h * d)
    K = (rng.standard_normal(shape) * 3).astype(np.float32)
    return np.zeros(shape, np.float32), K, rng.standard_normal(shape).astype(np.float32)


def _nan_int8(d, h, N, B):  # test_int8_nan_inputs: two NaNs each in Q, K and V (rows folded into N = 96)
    Q, K, V = inputs(N, h * d, B, "normal", 61)
    for X, pos in ((Q, [(3, 7), (68, 64)]), (K, [(0, 0), (37, 127)]), (V, [(72, 5), (31, 70)])):
        for r, col in pos:
            X[0, r, col] = np.nan
    return Q, K, V


HardCase = collections.namedtuple("HardCase", "name N B h int8_d f16_d build")
HARD_CASES = [
    HardCase("const", 288, 1, 2, (32, 64, 128), (64, 128), _const),  # nqb = 3: the pair loop's unpaired middle q-block
    HardCase("superdiag", 256, 2, 2, (32, 64, 128), (64, 128), _superdiag),
    HardCase("ramp", 512, 1, 2, (32, 64, 128), (64, 128), _ramp),
    HardCase("spike_tile", 256, 1, 2, (32, 64, 128), (64, 128), _spike_tile),
    HardCase("staircase", 512, 1, 2, (), (64, 128), _staircase),
    HardCase("underflow", 96, 1, 2, (64,), (64,), _underflow),
    HardCase("zero_q", 96, 2, 2, (32,), (128,), _zero_q),
    HardCase("nan_int8", 96, 1, 2, (64,), (), _nan_int8),
]
HARD = {c.name: c for c in HARD_CASES}
HARD_INT8 = [(c.name, d) for c in HARD_CASES for d in c.int8_d]
HARD_F16 = [(c.name, d) for c in HARD_CASES for d in c.f16_d]


def hard_inputs(name, d, **kw):
    """(Q, K, V) [B, N, h d] of a hard case at head size d; deterministic."""
    c = HARD[name]
    return c.build(d, c.h, c.N, c.B, **kw)


def prefix_mean(X):
    """float64 mean of rows 0..r of [B, N, C], for every r."""
    X = np.asarray(X, np.float64)
    return np.cumsum(X, axis=1) / np.arange(1, X.shape[1] + 1)[None, :, None]
