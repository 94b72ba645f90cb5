"""Numpy restatement of the sliding-window attend, and the inputs its CPU and GPU tests share.

Helper of tests/test_window_cpu.py and tests/test_gpu_window.py (not a test).  The token-granular call is the causal call on
zero-padded operands: Q at rows [s, s + Nq) of a zero block of Nq' = ceil32(s + Nq) rows, s = (L - Nq) mod
32, against L' = ceil32(L) key rows.  Under a window of W = 32 w rows, query group qg of the padded block, whose diagonal
tile is diag = qg + (L' - Nq') / 32, runs

  tiles   first = max(0, diag - w) ... diag from the zero state (m = 0, l = 0, O = 0), with the tile steps tests/split_ref.py
          restates (_int8_chunk, _f16_chunk): the int8 steps of causal_ref.fa_int8(base2=True), the fp16 steps of
          causal_ref.fa_fp16_lazy;
  masks   the diagonal tile hides key c from row r where c > r; tile diag - w, when it is >= 0, hides it where c <= r --
          the complement -- so that row r sees exactly the W keys (r - W, r] of its absolute position; the tiles between
          are unmasked.  A row's maximum over a tile it sees nothing of is -inf and leaves its state alone.

The private mutants (MUTANTS) let the CPU tests show that the inputs of the GPU tests would catch a wrong window:
no_left_mask (the left tile is unmasked), left_mask_inclusive (c >= r is visible: one key too many), first_off_by_one (the
sweep starts at diag - w + 1: the left tile is lost) and sweep_from_zero_tile (`first` is ignored: tiles 0 ... diag, the
left mask still on its tile).
"""
import numpy as np

from tests import causal_ref as cr
from tests import rect_ref as rr
from tests import split_ref as sr

INT8, F16 = sr.INT8, sr.F16
THR = sr.THR
GROUP = cr.GROUP
MUTANTS = ("no_left_mask", "left_mask_inclusive", "first_off_by_one", "sweep_from_zero_tile")
ceil32 = sr.ceil32
_IDX = np.arange(GROUP)


def geometry(L, Nq, window):
    """(s, Nq', L', diag_off, w) of a sequence of L rows attended by Nq rows under a window of `window` rows."""
    s = (L - Nq) % GROUP
    Nqp, Lp = ceil32(s + Nq), ceil32(L)
    return s, Nqp, Lp, (Lp - Nqp) // GROUP, window // GROUP


def first_tile(L, Nq, window, qg=0):
    """first(qg): the first tile query group qg computes."""
    _, _, _, off, w = geometry(L, Nq, window)
    return max(0, qg + off - w)


def first_row_staged(L, Nq, window):
    """64 * (first(0) / 2): the first cache row a windowed call may read -- the stage of the first group's first tile."""
    return 64 * (first_tile(L, Nq, window) // 2)


def _left_hidden(mutant):
    """[r][c] mask of the left tile: c <= r is hidden."""
    if mutant == "no_left_mask":
        return np.zeros((GROUP, GROUP), bool)
    if mutant == "left_mask_inclusive":
        return _IDX[None, :] < _IDX[:, None]
    return _IDX[None, :] <= _IDX[:, None]


def sweep(diag, w, mutant=None):
    """(tiles, left): the tiles a group with diagonal `diag` runs, and its left tile (negative: none)."""
    assert mutant is None or mutant in MUTANTS
    left = diag - w
    first = max(0, left)
    if mutant == "first_off_by_one":
        first = max(0, left + 1)
    if mutant == "sweep_from_zero_tile":
        first = 0
    return range(first, diag + 1), left


def _int8_group(Qg, sq, Kf, Vf, sK, sV, tiles, diag, left, hidden, d):
    """split_ref._int8_chunk's steps with the left tile's mask: (O, one-flip unit) of 32 rows."""
    f = np.float32
    c_log2 = cr.softmax_scale_log2(d)
    O, l, m, U = np.zeros((GROUP, d), f), np.zeros(GROUP, f), np.zeros(GROUP, f), np.zeros(GROUP, f)
    future = cr._future(None)
    for t in tiles:
        Kt, Vt = Kf[t * GROUP:(t + 1) * GROUP], Vf[t * GROUP:(t + 1) * GROUP]
        s = (Qg @ Kt.T).astype(f)
        c = f(f(sq * c_log2) * sK[t])
        if t == diag:
            s = np.where(future, f(-np.inf), s)
        if t == left:
            s = np.where(hidden, f(-np.inf), s)
        m_new = np.maximum(m, (s.max(axis=1) * c).astype(f)).astype(f)  # a row that sees nothing: max(m, -inf) = m
        p = np.exp2(cr._fma32(s, np.broadcast_to(c, s.shape), -m_new[:, None])).astype(f)
        alpha = np.exp2((m - m_new).astype(f)).astype(f)
        l = cr._fma32(alpha, l, cr._xor_tree_sum32(p))
        O = (O * alpha[:, None]).astype(f)
        m = m_new
        Pi, sP = cr._quantize_tile(p)
        ts = ((Pi @ Vt).astype(f) * sP).astype(f)
        O = cr._fma32(ts, np.broadcast_to(sV[t], ts.shape), O)
        U = np.maximum((U * alpha).astype(f), f(127.0) * sP * sV[t]).astype(f)
    ok = l > THR[INT8]
    lsafe = np.where(ok, l, f(1.0))
    return np.where(ok[:, None], (O / lsafe[:, None]).astype(f), f(0.0)), np.where(ok, U / lsafe, f(0.0))


def _f16_group(q, kk, v, tiles, diag, left, hidden, d):
    """split_ref._f16_chunk's steps with the left tile's mask: O of 32 rows."""
    f = np.float32
    c = cr.softmax_scale_log2(d)
    O, l, m = np.zeros((GROUP, d), f), np.zeros(GROUP, f), np.zeros(GROUP, f)
    future = cr._future(None)
    with np.errstate(over="ignore"):
        for t in tiles:
            kt, vt = kk[t * GROUP:(t + 1) * GROUP], v[t * GROUP:(t + 1) * GROUP]
            s = (q @ kt.T).astype(f)
            if t == diag:
                s = np.where(future, f(-np.inf), s)
            if t == left:
                s = np.where(hidden, f(-np.inf), s)
            p = np.exp2(cr._fma32(s, np.broadcast_to(c, s.shape), -m[:, None])).astype(f)
            ts = cr._quarter_sums(p)
            over = (ts > cr.LAZY_CAP).any(axis=1)  # a row that sees nothing has ts = 0: it never rebases
            if over.any():
                xm = (s[over].max(axis=1) * c).astype(f)
                alpha = np.exp2((m[over] - xm).astype(f)).astype(f)
                l[over] *= alpha
                O[over] *= alpha[:, None]
                m[over] = xm
                p[over] = np.exp2(cr._fma32(s[over], np.broadcast_to(c, s[over].shape), -xm[:, None])).astype(f)
                ts[over] = cr._quarter_sums(p[over])
            l = (l + ((ts[:, 0] + ts[:, 1]) + (ts[:, 2] + ts[:, 3]))).astype(f)
            O = (O + cr._half(p) @ vt).astype(f)
    ok = l > THR[F16]
    return np.where(ok[:, None], (O / np.where(ok, l, f(1.0))[:, None]).astype(f), f(0.0))


def attend(oracle, variant, Q, K, V, L, h, h_kv, window, mutant=None, unwindowed=False):
    """The windowed attend of one sequence, restated: Q [Nq, h d], K, V [>= L, h_kv d] float32.  Returns (O [Nq, h d],
    one-flip units [Nq, h d]; zeros for fp16).  unwindowed: split_ref's own tile steps over tiles 0 ... diag, the
    restatement of attend_tokens (the units are not formed)."""
    f = np.float32
    Nq, d = Q.shape[0], Q.shape[1] // h
    G = h // h_kv
    s, Nqp, Lp, off, w = geometry(L, Nq, window)
    Qp = np.zeros((1, Nqp, h * d), f)
    Qp[0, s:s + Nq] = Q
    Kp, Vp = (np.zeros((1, Lp, h_kv * d), f) for _ in range(2))
    Kp[0, :L], Vp[0, :L] = K[:L], V[:L]
    out, unit = np.zeros((Nq, h * d), f), np.zeros((Nq, h * d), f)
    if variant == INT8:
        (Qi, sQ), (Ki, sK), (Vi, sV) = oracle.quantize_heads(Qp, h * d, h), oracle.quantize_heads(Kp, h_kv * d, h_kv), \
            oracle.quantize_heads(Vp, h_kv * d, h_kv)
    hidden = _left_hidden(mutant)
    for k in range(h):
        kvh = k // G
        for qg in range(Nqp // GROUP):
            diag = qg + off
            rows = np.arange(qg * GROUP, (qg + 1) * GROUP) - s  # memory rows of the group's lanes
            real = (rows >= 0) & (rows < Nq)
            tiles, left = sweep(diag, w, mutant)
            u = None
            if variant == INT8:
                args = (Qi[0, k, qg * GROUP:(qg + 1) * GROUP].astype(f), sQ[0, k, qg], Ki[0, kvh].astype(f), Vi[0, kvh].astype(f),
                        sK[0, kvh], sV[0, kvh])
                if unwindowed:
                    o = sr._int8_chunk(*args, range(diag + 1), diag, d)[0]
                else:
                    o, u = _int8_group(*args, tiles, diag, left, hidden, d)
            else:
                args = (cr._half(Qp[0, qg * GROUP:(qg + 1) * GROUP, k * d:(k + 1) * d]), cr._half(Kp[0, :, kvh * d:(kvh + 1) * d]),
                        cr._half(Vp[0, :, kvh * d:(kvh + 1) * d]))
                o = sr._f16_chunk(*args, range(diag + 1), diag, d)[0] if unwindowed else _f16_group(*args, tiles, diag, left, hidden, d)
            out[rows[real], k * d:(k + 1) * d] = o[real]
            if u is not None:
                unit[rows[real], k * d:(k + 1) * d] = u[real][:, None]
    return out, unit


def attention_f64(Q, K, V, L, h, h_kv, window):
    """float64 attention of Q [Nq, h d] over the first L rows of K, V [.., h_kv d] under the band mask: row i sees the keys
    j with i + L - Nq - window < j <= i + L - Nq."""
    Q, K, V = (np.asarray(x, np.float64) for x in (Q, K[:L], V[:L]))
    Nq, d, G = Q.shape[0], Q.shape[1] // h, h // h_kv
    out = np.zeros_like(Q)
    pos = np.arange(Nq)[:, None] + (L - Nq)
    j = np.arange(L)[None, :]
    hidden = (j > pos) | (j <= pos - window)
    for k in range(h):
        kvh = k // G
        s = Q[:, k * d:(k + 1) * d] @ K[:, kvh * d:(kvh + 1) * d].T / np.sqrt(d)
        s = np.where(hidden, -np.inf, s)
        p = np.exp(s - s.max(-1, keepdims=True))
        out[:, k * d:(k + 1) * d] = (p / p.sum(-1, keepdims=True)) @ V[:, kvh * d:(kvh + 1) * d]
    return out


def keys_seen(L, Nq, window):
    """Per real row: how many keys it sees, min(window, i + L - Nq + 1)."""
    return np.minimum(window, np.arange(Nq) + L - Nq + 1)


within_bound = sr.within_bound

# ---- the inputs the GPU tests run, which tests/test_window_cpu.py shows to be inside the bounds and to catch the mutants -----
B, CAP = 3, 224  # Gk = 7: the last stage is partial
WINDOWS = (32, 64, 96)  # 32: the left tile is the diagonal's neighbour; 64 and 96: an even and an odd tile count
F64_WINDOWS = (64, 96)
# (lens, Nq) held to float64: every real row sees at least 33 keys before the window cuts, so at
# window >= 64 every row averages over min(window, 33 ...) keys
F64_SHAPES = [([95, 193, 224], 5), ([100, 160, 224], 32)]
HEADS = [(2, 2), (4, 2), (4, 1)]  # (h, h_kv)


def f64_seed(d, Nq, dist):
    return 9900 + 3 * d + 7 * Nq + (1 if dist == "uniform" else 0)


def random_inputs(d, h, h_kv, Nq, dist, seed):
    """Q [B, Nq, h d], K, V [B, CAP, h_kv d]: rect_ref.inputs' N(0, 0.25) or U[0, 1)."""
    Q, K, V = rr.inputs(Nq, CAP, h * d, B, dist, seed)
    return Q, np.ascontiguousarray(K[:, :, :h_kv * d]), np.ascontiguousarray(V[:, :, :h_kv * d])


def float64_inputs(built, heads=HEADS):
    """(label, variant, d, h, h_kv, window, lens, Nq, Q, K, V) of everything tests/test_gpu_window.py holds to float64, for the
    (variant, d) pairs of `built`: multi-head at every shape and distribution, grouped (h = 4 on 2 and 1 K/V heads) on the
    normal distribution at the first shape."""
    out = []
    for variant, d in built:
        for h, h_kv in heads:
            for lens, Nq in (F64_SHAPES if h == h_kv else F64_SHAPES[:1]):
                for dist in (("normal", "uniform") if h == h_kv else ("normal",)):
                    Q, K, V = random_inputs(d, h, h_kv, Nq, dist, f64_seed(d, Nq, dist) + 100 * h + h_kv)
                    for window in F64_WINDOWS:
                        out.append((f"{variant} d{d} h{h}/{h_kv} {dist} lens{lens} Nq{Nq} window{window}", variant, d, h, h_kv, window,
                                    lens, Nq, Q, K, V))
    return out
