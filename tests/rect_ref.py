"""References for rectangular attention (Nq != Nk), built from tests/causal_ref.py.

Helper of tests/test_rect_cpu.py, tests/test_rect_hard_cpu.py and tests/test_gpu_rect.py (not a test).  No
arithmetic is restated here: query groups are independent of each other and the K / V scales are per 32-row
group, so a rectangular result is a slice of a square one.
  * causal (bottom-right aligned, row r attends keys j <= r + Nk - Nq): Q goes into the LAST Nq rows of a zero
    [B, Nk, d_model] array, the square causal restatement runs at N = Nk, and the last Nq rows of its output
    (and of its one-flip units) are the answer.  Nk - Nq is a multiple of 32, so the zero rows fill whole
    query groups of their own and touch no scale of a real group.
  * non-causal: Q is fed in pieces of at most Nk rows, padded likewise, with causal=False.
The _mutant argument of causal_ref passes straight through.  With stats=True both restatements also return
causal_ref's branch statistics (did a query group re-anchor, did a row rebase?), sliced to the real query rows
like the output; the zero pad rows score 0 against every key, stay at m0 = 0 and take neither branch (asserted).

hard_inputs() cuts causal_ref's hard cases to a rectangle: the case is built at N = max(Nq, Nk) and Q keeps its
LAST Nq rows, K and V their first Nk, so a causal rectangular call is the last chunk of the square hard problem
at N = Nk.  HARD_INT8 / HARD_F16 list the shapes of DESIGN.md 11.3.
"""
import collections

import numpy as np

from tests import causal_ref as cr

# (Nq, Nk, d_model, h, B, causal): the smallest shapes at which each piece of the kernels' indexing can go wrong
CASES = [
    (32, 64, 64, 2, 1, True),     # d = 32; diagonal in the second slot of stage 0
    (32, 96, 128, 2, 1, True),    # diagonal opens a partial last stage
    (96, 160, 256, 2, 2, True),   # d = 128; three of four waves active; B = 2: Q/O and K/V batch strides differ
    (288, 352, 64, 2, 1, True),   # nqb = 3: the pair loop's unpaired middle q-block, second pass restarting
    (64, 224, 128, 1, 1, True),   # odd offset of 5 tiles; d = 128
    (160, 32, 128, 2, 2, False),  # Nq > Nk; one key tile; a second workgroup with one active wave; B = 2
    (32, 544, 64, 1, 1, False),   # one active wave; 17 tiles; odd tile count
    (160, 96, 256, 2, 1, False),  # Nq > Nk; d = 128; partial last stage without the mask
]
# fp16 only: the first and fourth case at a head size fa_tc_v1a is built for
CASES_F16_EXTRA = [
    (32, 64, 128, 2, 1, True),
    (288, 352, 128, 2, 1, True),
]
INT8_CASES = CASES
F16_CASES = [c for c in CASES if c[2] // c[3] in (64, 128)] + CASES_F16_EXTRA
DISTS = ("normal", "uniform")
# the shifted-superdiagonal shapes (Nq, Nk, d_model, h, B), all causal
SUPERDIAG = [(64, 160, 64, 2, 2), (64, 160, 128, 2, 2), (64, 160, 256, 2, 2), (96, 128, 128, 2, 1)]


def case_id(c):
    return f"Nq{c[0]}-Nk{c[1]}-d{c[2] // c[3]}-h{c[3]}-B{c[4]}-{'causal' if c[5] else 'full'}"


def seed_of(case, dist):
    Nq, Nk, d_model, h, B, causal = case
    return 7000 + Nq + 3 * Nk + 5 * d_model + 11 * h + 13 * B + (17 if causal else 0) + (1 if dist == "uniform" else 0)


def inputs(Nq, Nk, d_model, B, dist, seed):
    """Q [B, Nq, d_model], K and V [B, Nk, d_model]: causal_ref.inputs' N(0, 0.25) or U[0, 1)."""
    rng = np.random.default_rng(seed)
    shapes = [(B, Nq, d_model), (B, Nk, d_model), (B, Nk, d_model)]
    if dist == "normal":
        return [(rng.standard_normal(s) * 0.5).astype(np.float32) for s in shapes]
    return [rng.random(s, dtype=np.float32) for s in shapes]


def superdiag_inputs(Nq, Nk, d_model, B):
    """Shifted superdiagonal: the strongest key of query row r is r + Nk - Nq + 1, its first masked one."""
    rng = np.random.default_rng(300 + Nq + Nk + d_model)
    Q = (rng.standard_normal((B, Nq, d_model)) * 0.5).astype(np.float32)
    K = (rng.standard_normal((B, Nk, d_model)) * 0.5).astype(np.float32)
    K[:, Nk - Nq + 1:Nk] = 32.0 * Q[:, :Nq - 1]
    return Q, K, rng.standard_normal((B, Nk, d_model)).astype(np.float32)


def hard_inputs(name, d, Nq, Nk, **kw):
    """(Q [B, Nq, h d], K, V [B, Nk, h d]) of causal_ref.HARD[name] built at N = max(Nq, Nk), as copies."""
    c = cr.HARD[name]
    N = max(Nq, Nk)
    Q, K, V = c.build(d, c.h, N, c.B, **kw)
    return Q[:, N - Nq:].copy(), K[:, :Nk].copy(), V[:, :Nk].copy()


def zero_v_hard_inputs(d, Nq, Nk):
    """causal_ref.zero_v_inputs (V = 0) cut to a rectangle the same way, with `underflow`'s h and B."""
    c = cr.HARD["underflow"]
    N = max(Nq, Nk)
    Q, K, V = cr.zero_v_inputs(d, c.h, N, c.B)
    return Q[:, N - Nq:].copy(), K[:, :Nk].copy(), V[:, :Nk].copy()


# (name, Nq, Nk, causal) with the head sizes each variant runs it at; h and B are those of causal_ref.HARD[name]
HardShape = collections.namedtuple("HardShape", "name Nq Nk causal int8_d f16_d")
_ALL8, _ALL16 = (32, 64, 128), (64, 128)
HARD_SHAPES = [
    HardShape("const", 288, 352, True, _ALL8, _ALL16),       # nqb = 3, offset 2: every wave re-anchors on tile 0
    HardShape("spike_tile", 160, 256, True, _ALL8, _ALL16),  # nqb = 2, offset 3: pass 0 re-anchors, pass 1 restarts
    HardShape("ramp", 64, 512, True, _ALL8, _ALL16),         # 16 tiles: re-anchors on accumulated distance only
    HardShape("staircase", 64, 512, True, (), _ALL16),       # a rebase on every second tile of the loop
    HardShape("spike_tile", 64, 256, False, _ALL8, _ALL16),  # both branches without the mask, after four plain tiles
    HardShape("spike_tile", 288, 224, False, _ALL8, _ALL16),  # Nq > Nk, nqb = 3, Gk = 7: partial last stage
    HardShape("const", 160, 96, False, _ALL8, _ALL16),       # Nq > Nk, a second workgroup with one active wave
    HardShape("ramp", 32, 512, False, _ALL8, _ALL16),        # one active wave, accumulated re-anchor
    HardShape("staircase", 160, 224, False, (), _ALL16),
    HardShape("staircase", 32, 512, False, (), _ALL16),
    HardShape("underflow", 32, 96, True, (64,), (64,)),      # the guards: l under 1e-20 / 1e-10 gives exactly 0
    HardShape("underflow", 32, 96, False, (64,), (64,)),
    HardShape("underflow", 160, 96, False, (64,), (64,)),
    HardShape("zero_q", 64, 96, True, (32,), (128,)),        # B = 2; Q = 0: prefix mean / mean of V
    HardShape("zero_q", 64, 96, False, (32,), (128,)),
    HardShape("nan_int8", 32, 96, True, (64,), ()),          # one NaN in the Q slice (row 4), two each in K and V
    HardShape("nan_int8", 32, 96, False, (64,), ()),
]
HARD_INT8 = [(s, d) for s in HARD_SHAPES for d in s.int8_d]
HARD_F16 = [(s, d) for s in HARD_SHAPES for d in s.f16_d]


def hard_id(v):
    if isinstance(v, HardShape):
        return f"{v.name}-Nq{v.Nq}-Nk{v.Nk}-{'causal' if v.causal else 'full'}"
    return str(v)


def _batched(Q, K, V):
    Q, K, V = (np.ascontiguousarray(x, dtype=np.float32) for x in (Q, K, V))
    if Q.ndim == 2:
        return Q[None], K[None], V[None], True
    return Q, K, V, False


def _pieces(Nq, Nk, causal):
    """Row ranges of Q that one square run at N = Nk answers."""
    if causal:
        assert Nk >= Nq and (Nk - Nq) % cr.GROUP == 0
        return [(0, Nq)]
    return [(r0, min(r0 + Nk, Nq)) for r0 in range(0, Nq, Nk)]


def _padded(Q, r0, r1, Nk):
    """Rows r0..r1 of Q as the last rows of a zero [B, Nk, d_model] array."""
    P = np.zeros((Q.shape[0], Nk, Q.shape[2]), np.float32)
    P[:, Nk - (r1 - r0):] = Q[:, r0:r1]
    return P


def fa_int8(oracle, Q, K, V, d_model, h, causal=False, base2=False, _mutant=None, stats=False):
    """causal_ref.fa_int8 for Q [B, Nq, d_model] against K, V [B, Nk, d_model]: (O like Q, u [B, Nq, h]); with
    stats=True also causal_ref's Rise, each field [B, Nq, h] (a group's re-anchor counts stand on its 32 rows)."""
    Q, K, V, squeeze = _batched(Q, K, V)
    Nq, Nk = Q.shape[1], K.shape[1]
    out = np.zeros_like(Q)
    unit = np.zeros((Q.shape[0], Nq, h), np.float32)
    rise = cr.Rise(*(np.zeros((Q.shape[0], Nq, h), t) for t in (np.float32, bool, np.int64, bool)))
    for r0, r1 in _pieces(Nq, Nk, causal):
        pad = Nk - (r1 - r0)
        o, u, ri = cr.fa_int8(oracle, _padded(Q, r0, r1, Nk), K, V, d_model, h, causal=causal, base2=base2, _mutant=_mutant)
        out[:, r0:r1], unit[:, r0:r1] = o[:, pad:], u[:, pad:]
        for mine, theirs in zip(rise, ri):
            assert not theirs[:, :pad].any(), "a zero pad row rose or re-anchored"
            mine[:, r0:r1] = theirs[:, pad:]
    if squeeze:
        out, unit, rise = out[0], unit[0], cr.Rise(*(x[0] for x in rise))
    return (out, unit, rise) if stats else (out, unit)


def fa_fp16_lazy(oracle, Q, K, V, d_model, h, causal=False, _mutant=None, stats=False):
    """causal_ref.fa_fp16_lazy for Q [B, Nq, d_model] against K, V [B, Nk, d_model]: O like Q; with stats=True
    (O, rebased (row, tile) pairs, those on a diagonal tile), counted over the real query rows of every piece."""
    Q, K, V, squeeze = _batched(Q, K, V)
    Nq, Nk = Q.shape[1], K.shape[1]
    out = np.zeros_like(Q)
    rebased = on_diag = 0
    for r0, r1 in _pieces(Nq, Nk, causal):
        pad = Nk - (r1 - r0)
        o, n, nd = cr.fa_fp16_lazy(oracle, _padded(Q, r0, r1, Nk), K, V, d_model, h, causal=causal, _mutant=_mutant,
                                   per_row=True)
        assert not n[:, :pad].any() and not nd[:, :pad].any(), "a zero pad row rebased"
        out[:, r0:r1] = o[:, pad:]
        rebased, on_diag = rebased + int(n.sum()), on_diag + int(nd.sum())
    out = out[0] if squeeze else out
    return (out, rebased, on_diag) if stats else out


def attention_f64(Q, K, V, d_model, h, causal=False):
    """float64 softmax(Q K^T / sqrt(d)) V per head; causal: row r attends keys j <= r + Nk - Nq."""
    Q, K, V = (np.asarray(x, dtype=np.float64) for x in (Q, K, V))
    squeeze = Q.ndim == 2
    if squeeze:
        Q, K, V = Q[None], K[None], V[None]
    B, Nq, _ = Q.shape
    Nk, d = K.shape[1], d_model // h
    q = Q.reshape(B, Nq, h, d).transpose(0, 2, 1, 3)
    k, v = (x.reshape(B, Nk, h, d).transpose(0, 2, 1, 3) for x in (K, V))
    s = q @ k.transpose(0, 1, 3, 2) / np.sqrt(d)
    if causal:
        s = np.where(np.arange(Nk)[None, :] > np.arange(Nq)[:, None] + (Nk - Nq), -np.inf, s)
    s -= s.max(-1, keepdims=True)
    p = np.exp(s)
    p /= p.sum(-1, keepdims=True)
    o = (p @ v).transpose(0, 2, 1, 3).reshape(B, Nq, d_model)
    return o[0] if squeeze else o
