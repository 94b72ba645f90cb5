"""Numpy restatement of the split-KV attend, and the inputs its CPU and GPU tests share.

Helper of tests/test_split_cpu.py and tests/test_gpu_split.py (not a test).  The token-granular call is the causal call
on zero-padded operands: Q at rows [s, s + Nq) of a zero block of Nq' = ceil32(s + Nq) rows,
s = (L - Nq) mod 32, against L' = ceil32(L) key rows.  The split call cuts the key tiles of every 32-row query group qg
into chunks of C = chunk_rows / 32 tiles:

  partial   chunk c, c C <= last(qg) = qg + (L' - Nq') / 32, runs tiles c C ... min(c C + C - 1, last(qg)) from the zero
            state (m = 0, l = 0, O = 0) with causal_ref's tile steps -- the int8 steps of causal_ref.fa_int8(base2=True),
            the fp16 steps of causal_ref.fa_fp16_lazy -- and keeps Oc = O / l (0 under the variant's threshold), l and m;
  combine   per real row and head over the chunks c = 0 ... last(qg) // C, ascending, in float32:
            M = max m_c, a_c = l_c 2^(m_c - M), Ltot = sum a_c, O = Ltot > thr ? (sum a_c Oc_c) / Ltot : 0.

The scratch starts as NaN, so a combine that reads what no partial wrote shows.  combine() takes private mutants
(MUTANTS) so that the CPU tests can show the inputs of the GPU tests would catch a wrong combine.
"""
import numpy as np

from tests import causal_ref as cr
from tests import rect_ref as rr

INT8, F16 = "fa_tc_int8_b", "fa_tc_v1a"
THR = {INT8: np.float32(1e-20), F16: np.float32(1e-10)}
GROUP = cr.GROUP
# no_rescale: the weights are l_c, without 2^(m_c - M).  stale_max: M is chunk 0's m.  drop_chunk: the last chunk is
# not read.  read_beyond: one chunk past last(qg) // C is read, where the scratch holds what it held (NaN here).
MUTANTS = ("no_rescale", "stale_max", "drop_chunk", "read_beyond")


def ceil32(x):
    return -(-x // GROUP) * GROUP


def geometry(L, Nq, chunk_rows):
    """(s, Nq', L', diag_off, C) of a sequence of L rows attended by Nq rows."""
    s = (L - Nq) % GROUP
    Nqp, Lp = ceil32(s + Nq), ceil32(L)
    return s, Nqp, Lp, (Lp - Nqp) // GROUP, chunk_rows // GROUP


def chunks_read(L, Nq, chunk_rows):
    """Per real row r < Nq: how many chunks the combine reads, last(qg) // C + 1."""
    s, _, _, off, C = geometry(L, Nq, chunk_rows)
    return np.array([((s + r) // GROUP + off) // C + 1 for r in range(Nq)])


def _int8_chunk(Qg, sq, Kf, Vf, sK, sV, tiles, diag, d):
    """causal_ref.fa_int8(base2=True)'s tile steps over `tiles` from the zero state: (Oc, l, m) of 32 rows."""
    f = np.float32
    c_log2 = cr.softmax_scale_log2(d)
    O, l, m = np.zeros((GROUP, d), f), np.zeros(GROUP, f), np.zeros(GROUP, f)
    future = cr._future(None)
    for t in tiles:
        Kt, Vt = Kf[t * GROUP:(t + 1) * GROUP], Vf[t * GROUP:(t + 1) * GROUP]
        s = (Qg @ Kt.T).astype(f)
        c = f(f(sq * c_log2) * sK[t])
        if t == diag:
            s = np.where(future, f(-np.inf), s)
        m_new = np.maximum(m, (s.max(axis=1) * c).astype(f)).astype(f)
        p = np.exp2(cr._fma32(s, np.broadcast_to(c, s.shape), -m_new[:, None])).astype(f)
        alpha = np.exp2((m - m_new).astype(f)).astype(f)
        l = cr._fma32(alpha, l, cr._xor_tree_sum32(p))
        O = (O * alpha[:, None]).astype(f)
        m = m_new
        Pi, sP = cr._quantize_tile(p)
        ts = ((Pi @ Vt).astype(f) * sP).astype(f)
        O = cr._fma32(ts, np.broadcast_to(sV[t], ts.shape), O)
    ok = l > THR[INT8]
    return np.where(ok[:, None], (O / np.where(ok, l, f(1.0))[:, None]).astype(f), f(0.0)), l, m


def _f16_chunk(q, kk, v, tiles, diag, d):
    """causal_ref.fa_fp16_lazy's tile steps over `tiles` from the zero state (lazy base m0 = 0): (Oc, l, m) of 32 rows."""
    f = np.float32
    c = cr.softmax_scale_log2(d)
    O, l, m = np.zeros((GROUP, d), f), np.zeros(GROUP, f), np.zeros(GROUP, f)
    future = cr._future(None)
    with np.errstate(over="ignore"):  # p overflows to inf before a rebase, as in the kernel
        for t in tiles:
            kt, vt = kk[t * GROUP:(t + 1) * GROUP], v[t * GROUP:(t + 1) * GROUP]
            s = (q @ kt.T).astype(f)
            if t == diag:
                s = np.where(future, f(-np.inf), s)
            p = np.exp2(cr._fma32(s, np.broadcast_to(c, s.shape), -m[:, None])).astype(f)
            ts = cr._quarter_sums(p)
            over = (ts > cr.LAZY_CAP).any(axis=1)
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
    return np.where(ok[:, None], (O / np.where(ok, l, f(1.0))[:, None]).astype(f), f(0.0)), l, m


def partials(oracle, variant, Q, K, V, L, h, h_kv, chunk_rows, cap):
    """One sequence: Q [Nq, h d], K, V [>= L, h_kv d] float32.  Returns (Oc [NC, Nq, h d], m [NC, Nq, h], l [NC, Nq, h]) as
    the scratch holds them after the partial launch over a NaN-filled scratch: NaN where no chunk wrote."""
    f = np.float32
    Nq, d = Q.shape[0], Q.shape[1] // h
    G = h // h_kv
    s, Nqp, Lp, off, C = geometry(L, Nq, chunk_rows)
    NC = -(-cap // chunk_rows)
    Qp = np.zeros((1, Nqp, h * d), f)
    Qp[0, s:s + Nq] = Q
    Kp, Vp = (np.zeros((1, Lp, h_kv * d), f) for _ in range(2))
    Kp[0, :L], Vp[0, :L] = K[:L], V[:L]
    Oc = np.full((NC, Nq, h * d), np.nan, f)
    pm, pl = (np.full((NC, Nq, h), np.nan, f) for _ in range(2))
    if variant == INT8:
        (Qi, sQ), (Ki, sK), (Vi, sV) = oracle.quantize_heads(Qp, h * d, h), oracle.quantize_heads(Kp, h_kv * d, h_kv), \
            oracle.quantize_heads(Vp, h_kv * d, h_kv)
    for k in range(h):
        kvh = k // G
        for qg in range(Nqp // GROUP):
            last = qg + off
            rows = np.arange(qg * GROUP, (qg + 1) * GROUP) - s  # memory rows of the group's lanes
            real = (rows >= 0) & (rows < Nq)
            for c in range(last // C + 1):
                tiles = range(c * C, min(c * C + C - 1, last) + 1)
                if variant == INT8:
                    o, l, m = _int8_chunk(Qi[0, k, qg * GROUP:(qg + 1) * GROUP].astype(f), sQ[0, k, qg], Ki[0, kvh].astype(f),
                                          Vi[0, kvh].astype(f), sK[0, kvh], sV[0, kvh], tiles, last, d)
                else:
                    o, l, m = _f16_chunk(cr._half(Qp[0, qg * GROUP:(qg + 1) * GROUP, k * d:(k + 1) * d]),
                                         cr._half(Kp[0, :, kvh * d:(kvh + 1) * d]), cr._half(Vp[0, :, kvh * d:(kvh + 1) * d]), tiles, last, d)
                Oc[c, rows[real], k * d:(k + 1) * d] = o[real]
                pl[c, rows[real], k], pm[c, rows[real], k] = l[real], m[real]
    return Oc, pm, pl


def combine(variant, Oc, pm, pl, reads, mutant=None):
    """DESIGN.md 19.2 in float32 on partials [NC, Nq, ..]; reads [Nq]: the chunks each row reads.  O [Nq, h d]."""
    assert mutant is None or mutant in MUTANTS
    f = np.float32
    NC, Nq, h = pm.shape
    d = Oc.shape[2] // h
    out = np.zeros((Nq, h * d), f)
    for r in range(Nq):
        n = int(reads[r])
        if mutant == "drop_chunk":
            n = max(n - 1, 1)
        idx = list(range(n))
        for k in range(h):
            m = [pm[c, r, k] for c in idx]
            l = [pl[c, r, k] for c in idx]
            o = [Oc[c, r, k * d:(k + 1) * d] for c in idx]
            if mutant == "read_beyond":  # the entry behind the last one the partials wrote for this row
                beyond = n < NC
                m.append(pm[n, r, k] if beyond else f(np.nan))
                l.append(pl[n, r, k] if beyond else f(np.nan))
                o.append(Oc[n, r, k * d:(k + 1) * d] if beyond else np.full(d, np.nan, f))
            M = m[0] if mutant == "stale_max" else f(np.max(np.array(m, f)))
            Ltot, acc = f(0.0), np.zeros(d, f)
            with np.errstate(over="ignore", invalid="ignore"):
                for mc, lc, oc in zip(m, l, o):
                    a = lc if mutant == "no_rescale" else f(lc * np.exp2(f(mc - M)).astype(f))
                    Ltot = f(Ltot + a)
                    acc = cr._fma32(np.broadcast_to(a, oc.shape), oc, acc)
                out[r, k * d:(k + 1) * d] = (acc / Ltot).astype(f) if Ltot > THR[variant] else f(0.0)
                if np.isnan(Ltot):
                    out[r, k * d:(k + 1) * d] = np.nan
    return out


def attend(oracle, variant, Q, K, V, L, h, h_kv, chunk_rows, cap, mutant=None):
    """The split attend of one sequence, restated: O [Nq, h d] float32."""
    Oc, pm, pl = partials(oracle, variant, Q, K, V, L, h, h_kv, chunk_rows, cap)
    return combine(variant, Oc, pm, pl, chunks_read(L, Q.shape[0], chunk_rows), mutant)


def combine_f64(Oc, pm, pl, reads, thr):
    """DESIGN.md 19.2 evaluated in float64 on float32 partials [NC, Nq, ..] (what the GPU left in its scratch); also the
    per-element bound of tests/test_gpu_split.py's combine test: (2 n_c + 4) 2^-23 max_c |Oc_c| over the row's chunks."""
    NC, Nq, h = pm.shape
    d = Oc.shape[2] // h
    out, bound = np.zeros((Nq, h * d)), np.zeros((Nq, h * d))
    for r in range(Nq):
        n = int(reads[r])
        for k in range(h):
            m, l = pm[:n, r, k].astype(np.float64), pl[:n, r, k].astype(np.float64)
            o = Oc[:n, r, k * d:(k + 1) * d].astype(np.float64)
            a = l * np.exp2(m - m.max())
            Ltot = a.sum()
            out[r, k * d:(k + 1) * d] = (a[:, None] * o).sum(axis=0) / Ltot if Ltot > float(thr) else 0.0
            bound[r, k * d:(k + 1) * d] = (2 * n + 4) * 2.0 ** -23 * np.abs(o).max(axis=0)
    return out, bound


def attention_f64(Q, K, V, L, h, h_kv):
    """float64 attention of Q [Nq, h d] over the first L rows of K, V [.., h_kv d], causal and bottom-right aligned."""
    Q, K, V = (np.asarray(x, np.float64) for x in (Q, K[:L], V[:L]))
    Nq, d, G = Q.shape[0], Q.shape[1] // h, h // h_kv
    out = np.zeros_like(Q)
    for k in range(h):
        kvh = k // G
        s = Q[:, k * d:(k + 1) * d] @ K[:, kvh * d:(kvh + 1) * d].T / np.sqrt(d)
        s = np.where(np.arange(L)[None, :] > np.arange(Nq)[:, None] + (L - Nq), -np.inf, s)
        p = np.exp(s - s.max(-1, keepdims=True))
        out[:, k * d:(k + 1) * d] = (p / p.sum(-1, keepdims=True)) @ V[:, kvh * d:(kvh + 1) * d]
    return out


def within_bound(variant, got, ref):
    """The accuracy contract of DESIGN.md 17.1: int8 within 5e-3, fp16 within max(1e-3, 1e-3 |ref|), of float64."""
    err = np.abs(got.astype(np.float64) - ref)
    if variant == INT8:
        return np.isfinite(got).all() and bool((err <= 5e-3).all())
    return np.isfinite(got).all() and bool((err <= np.maximum(1e-3, 1e-3 * np.abs(ref))).all())


# ---- the inputs the GPU tests run, which tests/test_split_cpu.py shows to be inside the bounds and to catch the mutants -----
B, CAP = 3, 224  # the last stage and the last chunk are partial
CHUNKS = (64, 128)
# (lens, Nq) whose rows all see at least 33 keys: the rows the float64 bounds are asked of (tests/test_tokens_cpu.py)
F64_SHAPES = [([95, 193, 224], 5), ([100, 160, 224], 32)]
# Climbing maxima, one sequence of L = cap = HARD_CAP rows attended by its last HARD_NQ rows (causal_ref.HARD_CASES):
#   HARD_F64      the fp16 ramp at d = 128: the chunks' m climb by more than 48 log2 units and the result stays inside the
#                 float64 bound (the int8 ramp and both staircases do not: their rows weigh a handful of keys, so V's
#                 quantisation / P's rounding does not average out -- 2.5e-2 and 5e-3, with or without a split);
#   HARD_COMBINE  the staircase: m climbs by more than 128 log2 units.  M cancels between numerator and denominator, so a
#                 wrong M ("stale_max") changes nothing until a weight l_c 2^(m_c - M) overflows fp32, which takes such a
#                 climb; these run the tests of the combine pass alone, which ask nothing of the attention's accuracy.
HARD_F64 = (F16, 128, "ramp")
HARD_COMBINE = [(INT8, 64, "staircase"), (F16, 64, "staircase")]
HARD_CAP, HARD_NQ = 512, 5


def f64_seed(d, Nq, dist):
    return 9500 + 3 * d + 7 * Nq + (1 if dist == "uniform" else 0)


def random_inputs(d, h, h_kv, Nq, dist, seed):
    """Q [B, Nq, h d], K, V [B, CAP, h_kv d]: rect_ref.inputs' N(0, 0.25) or U[0, 1)."""
    Q, K, V = rr.inputs(Nq, CAP, h * d, B, dist, seed)
    return Q, np.ascontiguousarray(K[:, :, :h_kv * d]), np.ascontiguousarray(V[:, :, :h_kv * d])


def hard_inputs(name, d):
    """(Q [HARD_NQ, h d], K, V [HARD_CAP, h d], h) of a climbing-maxima case: the last rows attend the whole sequence."""
    Q, K, V = rr.hard_inputs(name, d, HARD_NQ, HARD_CAP)
    return Q[0], K[0], V[0], cr.HARD[name].h


def float64_inputs(built):
    """(label, variant, h, h_kv, chunk, [(Q, K, V, L) per sequence], cap) of everything tests/test_gpu_split.py holds to
    float64, for the (variant, d) pairs of `built`; tests/test_split_cpu.py holds the restatement to the same bounds."""
    out = []
    for variant, d in built:
        for lens, Nq in F64_SHAPES:
            for dist in ("normal", "uniform"):
                Q, K, V = random_inputs(d, 2, 2, Nq, dist, f64_seed(d, Nq, dist))
                for chunk in CHUNKS:
                    out.append((f"{variant} d{d} {dist} lens{lens} Nq{Nq} chunk{chunk}", variant, 2, 2, chunk,
                                [(Q[b], K[b], V[b], L) for b, L in enumerate(lens)], CAP))
    variant, d, name = HARD_F64
    Q, K, V, h = hard_inputs(name, d)
    for chunk in CHUNKS:
        out.append((f"{variant} d{d} {name} chunk{chunk}", variant, h, h, chunk, [(Q, K, V, HARD_CAP)], HARD_CAP))
    return out
