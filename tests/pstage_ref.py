"""The P stage of the per-block int8 kernels, tile by tile: restatements and checkers.

Helper of tests/test_pstage_cpu.py and tests/test_gpu_pstage.py (not a test).  qmha_debug_fa_int8_pstage runs the
dumping twin of a shipped kernel and returns, for every tile a wave computes, what the kernel held: S, Qi, sQ, the
running max m, the P scale sP, the quantised Pi as the P@V MFMA read it, the integer accumulator T, and the row sum
l.  restate() computes the same record in float32 numpy, step for step as the sources have it, plus x = p / sP
before rounding, and the check_* functions hold a dump (from the GPU, or a synthetic one) to that record.

Three forms (restate's `form`):
  "base2"  qmha_fa_int8_masked_kernel and qmha_fa_int8_kernel: c = (sQ c_log2) sK, m = max(m, RN(mx c)),
           p = exp2(fma(S, c, -m)), sP = max(pmax / 127, 1e-8), Pi = rint(p (1 / sP)).  This is
           causal_ref.fa_int8(base2=True); the two kernels differ from it, and from each other, only in how the
           quotient and the reciprocal are formed (div127_fast, rcp_fast) and in the anchored fold, neither of which
           the record depends on (C, D, F and G below carry their error).
  "nats"   the C oracle's score arithmetic (causal_ref.fa_int8(base2=False)); no kernel, the restatement's anchor.
  "kfold"  qmha_fa_int8_pipe_kernel (FL_KFOLD): c' = c rounded to 22 bits, m = max(m, RN(Smax c')),
           Kn = fma(c', 1.5 2^23, m), f = fma(fma(c', -1.5 2^23, Kn) - m, ln 2, 1), p' = exp2(fma(A, c', -Kn)) on the
           biased accumulator A = 1.5 2^23 + S, sP = max(pmax, 1.27e-6) (1/127) with pmax = exp2(fma(Smax, c', -m)),
           Pi = rint(p' ((1 / sP) f)); the row sum is sum(p') f.

Rounding units below: u = 2^-24 (one float32 rounding, relative) and e = 2^-23 (one float32 ulp, relative, at
most).  The hardware's v_exp_f32 and v_rcp_f32 are documented to 1 ulp (AMD CDNA3 / CDNA4 ISA guides); numpy's
float32 exp2 (the C library's exp2f) is held to 0.5 ulp + 2^-9 ulp, taken as 0.5 e.

What is exact (no tolerance): A (S, Qi, sQ), B (m: one float32 multiply and a max on exact integers), E (T = Pi Vi on
the kernel's own Pi), H (what is not computed is not written).  What is bounded, and by what:

C. sP, relative.  The exponent of pmax is the same float32 in both (B).  exp2: e (GPU) + 0.5 e (here).  base2: the
   quotient here is correctly rounded (u = 0.5 e), div127_fast is the correctly rounded quotient except for double
   roundings (e).  kfold: both multiply by RN(1/127); two results of one rounding each whose inputs differ move by
   at most 2 u = e beyond the inputs' difference.  EPS_SP = 3 e (base2), 2.5 e (kfold).  max(., floor) does not
   expand.  Where this restatement's unfloored value lies below floor (1 - EPS_SP), the GPU's must be the floor
   exactly.
D. Pi.  x = p inv with inv = 1 / sP (times f in kfold).  Relative: p 1.5 e (as pmax); sP EPS_SP <= 3 e; the
   reciprocal 0.5 e here (correctly rounded), e on the GPU (v_rcp_f32, or rcp_fast which is no worse): 1.5 e; kfold's
   product with f, one rounding each side: e (base2 has instead the oracle's float32 product p inv before rint,
   0.5 e: smaller); the GPU's fma rounds the exact product once, to the integer.  Sum: 1.5 + 3 + 1.5 + 1 = 7 e,
   on x <= 127 f with f <= 1.004 (asserted): DELTA = 7 * 2^-23 * 127.5 = 1.064e-4 in units of x.  Where x here is
   farther than DELTA from every half-integer, Pi must be equal; within DELTA it may differ by exactly 1.  With x
   equidistributed near the boundaries the excused share is about 2 DELTA = 2.1e-4; MAX_EXCUSED_SHARE = 1e-3 caps
   it per case, and the CPU tests assert that the restatement's own near-boundary share stays under the cap.
F. l, relative to the float64 sum over tiles of 2^(m_t - m_final) sum_j p_tj (f_t), p from here, m the kernel's own.
   p: 1.5 e.  The tile's shift exp2(m_t - anchor): e, its product with f (kfold): u.  Summation of positive terms:
   a 16-term tree (4 roundings), one fma per tile (Gk), the join of the two key halves (1), the final multiply (1):
   (Gk + 6) u.  Each re-anchor multiplies by an exp2: (e + u) each, R of them (R counted from m by the kernel's
   own rule: any row of the group more than 48 above the anchor); the final un-anchor likewise (e + u).
   EPS_L = (7.5 + Gk / 2 + 1.5 R) e, plus 32 Gk 2^-126 absolute for subnormal p the hardware flushes.
G. O, per element, against the float64 replay of the kernel's OWN dump, sum_t T_t sP_t sV_t 2^(m_t - m_final) / l:
   with A the same sum over |T_t|, |O - replay| <= EPS_O A.  The tile's scale (sP 2^24) sV 2^(m_t - anchor): two
   roundings and an exp2, 2 u + e; one fma rounding per fold, each on a partial sum of magnitude <= A: Gk u; R
   re-anchors (e + u) each; the un-anchor multiply (e + u); the division u; the drain's multiply-add u.
   EPS_O = (5 + Gk / 2 + 1.5 R) e.  Rows with l <= 1e-20 are exactly 0.
"""
import collections

import numpy as np

from tests import causal_ref as cr
from tests import rect_ref as rr

GROUP = cr.GROUP
F = np.float32
E_ULP = 2.0 ** -23
EPS_SP = {"base2": 3.0 * E_ULP, "kfold": 2.5 * E_ULP}
F_MAX = 1.004
DELTA = 7.0 * E_ULP * 127.5
MAX_EXCUSED_SHARE = 1e-3
MAGIC = F(12582912.0)  # 1.5 * 2^23
FLOOR = {"base2": F(1e-8), "nats": F(1e-8), "kfold": F(F(1.27e-6) * (F(1.0) / F(127.0)))}
REANCHOR = 48.0
# key of accumulator register r of lane half hh (qmha_common.hpp acc_row); P@V k-step ks holds registers 8 ks .. +7
ACC_ROW = np.array([[(r & 3) + 8 * (r >> 2) + 4 * hh for r in range(16)] for hh in range(2)])
MUTANTS = (None, "sp_unmasked")


# ---- the committed cases: the smallest shapes that reach each code path (tests/test_gpu_pstage.py runs them on the
# GPU, tests/test_pstage_cpu.py holds the restatement alone to D's cap on every one)
Case = collections.namedtuple("Case", "label kind d_model h causal build")  # build() -> (Q, K, V)


def form_of(case_or_kind):
    """pstage_ref's form of a kernel: the pipelined kernel is the only KFOLD one."""
    kind = getattr(case_or_kind, "kind", case_or_kind)
    return "kfold" if kind == "pipe" else "base2"


def kind_of(Nq, Nk, d, causal):
    """Which main kernel run() launches for a fa_tc_int8_b call (qmha_api.cpp, fa_int8_d, fa_int8_pipe_launch)."""
    if causal or Nq != Nk:
        return "masked"
    return "pipe" if d in (32, 64, 128) and Nk >= 64 else "one-tile"


def _square(N, d, h, B, dist):
    return lambda: cr.inputs(N, h * d, B, dist, 9000 + N + 7 * d + 31 * h + 101 * B + (1 if dist == "uniform" else 0))


def _cases():
    out = []
    # the pipelined kernel: N = 64 prologue and epilogue only; 96 an odd tile count, a partial last stage, three of
    # four waves; 224 one period of the 3-slot x 2-tile ring plus one; 416 two periods plus one; both distributions
    # at 7 tiles; different data per (batch, head) slice; l over 32 tiles
    pipe = [(N, d, 1, 1, "uniform" if (N // 32 + d // 32) % 2 else "normal") for d in (32, 64, 128) for N in (64, 96, 224, 416)]
    pipe += [(224, d, 1, 1, "normal" if (7 + d // 32) % 2 else "uniform") for d in (32, 64, 128)]
    pipe += [(96, 64, 2, 2, "normal"), (1024, 64, 1, 1, "normal")]
    for N, d, h, B, dist in pipe:
        out.append(Case(f"pipe-N{N}-d{d}-h{h}-B{B}-{dist}", "pipe", h * d, h, False, _square(N, d, h, B, dist)))
    # the one-tile kernel: every other head size, and N = 32 of the pipelined ones
    for N, d, dist in ((96, 96, "normal"), (96, 256, "uniform"), (32, 64, "normal")):
        out.append(Case(f"one-tile-N{N}-d{d}-{dist}", "one-tile", 2 * d, 2, False, _square(N, d, 2, 1, dist)))
    # the masked kernel, both geometries: causal_ref's and rect_ref's shapes up to N = 288 / Nk = 352
    for N, d_model, h, B, dist, seed in cr.CASES + cr.CASES_INT8_D32:
        if N <= 288:
            out.append(Case(f"causal-N{N}-d{d_model // h}-h{h}-B{B}-{dist}", "masked", d_model, h, True,
                            lambda a=(N, d_model, B, dist, seed): cr.inputs(*a)))
    for c in rr.CASES:
        for dist in rr.DISTS:
            if c[1] <= 352:
                out.append(Case(f"rect-{rr.case_id(c)}-{dist}", "masked", c[2], c[3], c[5],
                                lambda c=c, dist=dist: rr.inputs(c[0], c[1], c[2], c[4], dist, rr.seed_of(c, dist))))
    # hard inputs (causal_ref.HARD): the ramp and the spike tile re-anchor (on and off the diagonal; in the pipelined
    # kernel the pending tile's scale_prev takes the factor too), underflow sits on the sP floor and the l guard,
    # zero Q, NaN inputs.  d = 64, the ramp and the spike at 32 and 128 too; the one-tile kernel at d = 96.
    hard = [(n, d) for n in ("ramp", "spike_tile") for d in (32, 64, 128)] + [(n, 64) for n in ("underflow", "zero_q", "nan_int8")]
    for kind, causal, sizes in (("pipe", False, hard), ("masked", True, hard),
                                ("one-tile", False, [(n, 96) for n in ("ramp", "spike_tile", "underflow", "zero_q", "nan_int8")])):
        for name, d in sizes:
            out.append(Case(f"hard-{kind}-{name}-d{d}", kind, cr.HARD[name].h * d, cr.HARD[name].h, causal,
                            lambda a=(name, d): cr.hard_inputs(*a)))
    return out


CASES = _cases()
# the hard cases that take the re-anchor branch (the ramp at d = 32 tops out at m = 38.8 log2 units, under the 48)
REANCHORS = {c.label for c in CASES if c.label.startswith("hard-") and ("-ramp-" in c.label or "-spike_tile-" in c.label)
             and not c.label.endswith("-ramp-d32")}


def geometry(Nq, Nk, causal):
    """(Gq, Gk, last[g]): group g computes key tiles t <= last[g]; causal is bottom-right aligned."""
    Gq, Gk = Nq // GROUP, Nk // GROUP
    off = Gk - Gq if causal else Gk
    assert off >= 0
    return Gq, Gk, np.minimum(np.arange(Gq) + off, Gk - 1)


def visited(Nq, Nk, causal):
    """[Gq, Gk] bool: the tiles a wave must compute."""
    Gq, Gk, last = geometry(Nq, Nk, causal)
    return np.arange(Gk)[None, :] <= last[:, None]


def _c22(c):
    """FL_KFOLD's score scale: c rounded to 22 significant bits, (bits + 2) & ~3."""
    return ((np.asarray(c, F).view(np.int32) + 2) & ~3).view(F)


def restate(oracle, Q, K, V, d_model, h, form="base2", causal=False, _mutant=None):
    """The per-tile record of one call.  Q [B, Nq, d_model], K and V [B, Nk, d_model].

    Returns a dict in the dump's layouts (Gq = Nq / 32, Gk = Nk / 32): S [B, h, Nq, Nk] int32, Qi, sQ, m
    [B, h, Nq, Gk], sP [B, h, Gq, Gk], Pi [B, h, Nq, Nk] int8, T [B, h, Gk, Nq, d] int32, l [B, h, Nq], O like Q;
    plus x [B, h, Nq, Nk] float64 (p inv before rounding), p [B, h, Nq, Nk] float32, f [B, h, Nq, Gk] (1 outside
    kfold), sP_raw (sP before its floor), visited [Gq, Gk], Vi, sV and the form.  Entries of tiles that are not
    computed are 0.  O and l follow causal_ref.fa_int8's alpha form in float32 (bit for bit in "base2" / "nats").
    _mutant="sp_unmasked" (tests only): the diagonal tile's sP formed over the scores before the mask."""
    assert form in FLOOR and _mutant in MUTANTS
    Q, K, V = (np.ascontiguousarray(a, dtype=F) for a in (Q, K, V))
    B, Nq, _ = Q.shape
    Nk, d = K.shape[1], d_model // h
    Gq, Gk, last = geometry(Nq, Nk, causal)
    off = Gk - Gq if causal else Gk
    (Qi, sQ), (Ki, sK), (Vi, sV) = (oracle.quantize_heads(a, d_model, h) for a in (Q, K, V))
    c_log2, inv_sqrt_d = cr.softmax_scale_log2(d), F(1.0) / np.sqrt(F(d))
    future = cr._future(None)
    rec = dict(S=np.zeros((B, h, Nq, Nk), np.int32), Qi=Qi, sQ=sQ, m=np.zeros((B, h, Nq, Gk), F),
               sP=np.zeros((B, h, Gq, Gk), F), sP_raw=np.zeros((B, h, Gq, Gk), F), Pi=np.zeros((B, h, Nq, Nk), np.int8),
               T=np.zeros((B, h, Gk, Nq, d), np.int32), l=np.zeros((B, h, Nq), F), O=np.zeros_like(Q),
               x=np.zeros((B, h, Nq, Nk)), p=np.zeros((B, h, Nq, Nk), F), f=np.ones((B, h, Nq, Gk), F),
               visited=visited(Nq, Nk, causal), Vi=Vi, sV=sV, form=form, causal=causal)
    for b in range(B):
        for k in range(h):
            S = Qi[b, k].astype(np.int32) @ Ki[b, k].astype(np.int32).T
            rec["S"][b, k] = S
            Vf = Vi[b, k].astype(np.int32)
            O = np.zeros((Nq, d), F)
            l = np.zeros(Nq, F)
            m_prev = np.zeros(Nq, F)  # m0 = 0
            for t in range(Gk):
                g0 = max(0, t - off)  # the first group that computes tile t; its diagonal one if t - off >= 0
                r0 = g0 * GROUP
                if r0 >= Nq:
                    break
                cols = slice(t * GROUP, (t + 1) * GROUP)
                acc = S[r0:, cols].astype(F)  # exact
                sq = np.repeat(sQ[b, k, g0:], GROUP)
                diag = causal and t - off >= 0
                fac = np.ones(Nq - r0, F)
                if form == "nats":
                    s = ((acc * sq[:, None]).astype(F) * sK[b, k, t]).astype(F)
                    s = (s * inv_sqrt_d).astype(F)
                else:
                    s = acc
                    c = ((sq * c_log2).astype(F) * sK[b, k, t]).astype(F)
                    if form == "kfold":
                        c = _c22(c)
                raw = s
                if diag:
                    s = s.copy()
                    s[:GROUP] = np.where(future, F(-np.inf), s[:GROUP])
                mx = s.max(axis=1)
                if form == "nats":
                    m_new = np.maximum(m_prev[r0:], mx).astype(F)
                    e = lambda z: np.exp((z - m_new[:, None]).astype(F)).astype(F)
                elif form == "base2":
                    m_new = np.maximum(m_prev[r0:], (mx * c).astype(F)).astype(F)
                    e = lambda z: np.exp2(cr._fma32(z, np.broadcast_to(c[:, None], z.shape), -m_new[:, None])).astype(F)
                else:
                    m_new = np.maximum(m_prev[r0:], (mx * c).astype(F)).astype(F)
                    kn = cr._fma32(c, np.broadcast_to(MAGIC, c.shape), m_new)
                    delta = (cr._fma32(c, np.broadcast_to(-MAGIC, c.shape), kn) - m_new).astype(F)
                    fac = cr._fma32(delta, np.broadcast_to(F(0.69314718055994531), delta.shape), np.ones_like(delta))
                    assert fac.max() <= F_MAX and fac.min() >= 2.0 - F_MAX, "KFOLD row factor outside DELTA's premise"
                    # the biased accumulator is exact in float32 (|S| < 2^22); -inf stays -inf
                    e = lambda z: np.exp2(cr._fma32((z + MAGIC).astype(F), np.broadcast_to(c[:, None], z.shape), -kn[:, None])).astype(F)
                p = e(s)
                # the tile's largest p, by row: the kernels' pmax is the exp of the row max (kfold: its own fma)
                top = np.exp2(cr._fma32(mx, c, -m_new)).astype(F) if form == "kfold" else p.max(axis=1)
                if diag and _mutant == "sp_unmasked":
                    top = top.copy()
                    top[:GROUP] = e(raw)[:GROUP].max(axis=1) if form != "kfold" else np.exp2(
                        cr._fma32(raw[:GROUP].max(axis=1), c[:GROUP], -m_new[:GROUP])).astype(F)
                pmax = top.reshape(-1, GROUP).max(axis=1)
                if form == "kfold":
                    sp_raw = (pmax * (F(1.0) / F(127.0))).astype(F)
                    sp = (np.maximum(pmax, F(1.27e-6)) * (F(1.0) / F(127.0))).astype(F)
                    inv = ((F(1.0) / sp).astype(F).repeat(GROUP) * fac).astype(F)
                    x = p.astype(np.float64) * inv[:, None].astype(np.float64)
                    Pi = np.rint(x)
                else:
                    sp_raw = (pmax / F(127.0)).astype(F)
                    sp = np.maximum(sp_raw, F(1e-8)).astype(F)
                    inv = (F(1.0) / sp).astype(F).repeat(GROUP)
                    x = p.astype(np.float64) * inv[:, None].astype(np.float64)
                    Pi = np.clip(np.rint((p * inv[:, None]).astype(F)), -128, 127)  # oracle_quantize_block
                T = Pi.astype(np.int32) @ Vf[cols]
                # causal_ref.fa_int8's alpha form
                ex = np.exp if form == "nats" else np.exp2
                alpha = ex((m_prev[r0:] - m_new).astype(F)).astype(F)
                rowsum = cr._xor_tree_sum32(p)
                if form == "kfold":
                    rowsum = (rowsum * fac).astype(F)
                l[r0:] = cr._fma32(alpha, l[r0:], rowsum)
                ts = (T.astype(F) * sp.repeat(GROUP)[:, None]).astype(F)
                O[r0:] = cr._fma32(ts, np.broadcast_to(sV[b, k, t], ts.shape), (O[r0:] * alpha[:, None]).astype(F))
                m_prev[r0:] = m_new
                rec["m"][b, k, r0:, t] = m_new
                rec["f"][b, k, r0:, t] = fac
                rec["sP"][b, k, g0:, t], rec["sP_raw"][b, k, g0:, t] = sp, sp_raw
                rec["Pi"][b, k, r0:, cols], rec["x"][b, k, r0:, cols], rec["p"][b, k, r0:, cols] = Pi, x, p
                rec["T"][b, k, t, r0:] = T
            ok = l > F(1e-20)
            lsafe = np.where(ok, l, F(1.0))
            rec["l"][b, k] = l
            rec["O"][b, :, k * d:(k + 1) * d] = np.where(ok[:, None], (O / lsafe[:, None]).astype(F), F(0.0))
    return rec


# ---- the float64 views F and G compare against ------------------------------------------------------------
def _tile_mask(rec):
    """visited, spread to [1, 1, Nq, Gk]."""
    return np.repeat(rec["visited"], GROUP, axis=0)[None, None]


def m_final(m, rec):
    """[B, h, Nq]: the running max after a row's last computed tile."""
    last = np.repeat(rec["visited"].sum(axis=1) - 1, GROUP)
    return np.take_along_axis(m, np.broadcast_to(last[None, None, :, None], m.shape[:3] + (1,)), axis=3)[..., 0]


def _shift(m, rec):
    """[B, h, Nq, Gk] float64: 2^(m_t - m_final) on computed tiles, 0 elsewhere."""
    m = m.astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        return np.where(_tile_mask(rec), np.exp2(m - m_final(m, rec)[..., None]), 0.0)


def l_f64(rec, m):
    """The row sum from the restatement's p and row factors, shifted by the max record m (the kernel's own)."""
    B, h, Nq, Nk = rec["p"].shape
    tile_sums = rec["p"].astype(np.float64).reshape(B, h, Nq, Nk // GROUP, GROUP).sum(-1) * rec["f"]
    return (tile_sums * _shift(m, rec)).sum(-1)


def replay_f64(dump, rec):
    """(O [B, Nq, d_model], A likewise) in float64 from a dump's own T, sP, m and l and the inputs' sV."""
    T = dump["T"].astype(np.float64)  # [B, h, Gk, Nq, d]
    B, h, Gk, Nq, d = T.shape
    scale = np.repeat(dump["sP"].astype(np.float64), GROUP, axis=2) * rec["sV"].astype(np.float64)[:, :, None, :]
    w = (scale * _shift(dump["m"], rec)).transpose(0, 1, 3, 2)[..., None]  # [B, h, Gk, Nq, 1]
    w = np.where(_tile_mask(rec).transpose(0, 1, 3, 2)[..., None], w, 0.0)
    T = np.where(_tile_mask(rec).transpose(0, 1, 3, 2)[..., None], T, 0.0)
    l = dump["l"].astype(np.float64)
    ok = l > 1e-20
    lsafe = np.where(ok, l, 1.0)[..., None]
    num, mag = (T * w).sum(2) / lsafe, (np.abs(T) * w).sum(2) / lsafe
    num, mag = np.where(ok[..., None], num, 0.0), np.where(ok[..., None], mag, 0.0)
    return tuple(a.transpose(0, 2, 1, 3).reshape(B, Nq, h * d) for a in (num, mag))


def reanchors(m, rec):
    """[B, h, Gq]: how often a group re-anchors (any of its rows more than 48 above the anchor; anchor0 = 0)."""
    B, h, Nq, Gk = m.shape
    mg = m.reshape(B, h, Nq // GROUP, GROUP, Gk)
    anchor = np.zeros(mg.shape[:4], F)
    count = np.zeros(mg.shape[:3], np.int64)
    for t in range(Gk):
        on = rec["visited"][None, None, :, t]
        hit = on & ((mg[..., t] - anchor) > F(REANCHOR)).any(axis=-1)
        anchor = np.where(hit[..., None], mg[..., t], anchor)
        count += hit
    return count


def as_dump(rec):
    """The record presented as a dump: the kernel's fields, with l and O taken from the float64 views."""
    dump = {k: rec[k].copy() for k in ("S", "Qi", "sQ", "m", "sP", "Pi", "T")}
    return finish_dump(dump, rec)


def finish_dump(dump, rec):
    """Give a synthetic dump the l and O that belong to its own m, sP and T."""
    dump["l"] = l_f64(rec, dump["m"]).astype(F)
    dump["O"] = replay_f64(dump, rec)[0].astype(F)
    return dump


# ---- checkers: each raises AssertionError naming its letter, or returns what it observed --------------------
def _fail(letter, what):
    raise AssertionError(f"{letter}: {what}")


def _eq_on(letter, name, got, want, mask):
    bad = mask & (got != want)
    if bad.any():
        i = tuple(int(v) for v in np.argwhere(bad)[0])
        _fail(letter, f"{name}{list(i)} = {got[i]!r}, expected {want[i]!r} ({int(bad.sum())} mismatches)")


def check_A(dump, rec):
    """S, Qi, sQ bit-exact (S where its tile is computed)."""
    el = np.repeat(_tile_mask(rec), GROUP, axis=3)
    _eq_on("A", "S", dump["S"], rec["S"], np.broadcast_to(el, rec["S"].shape))
    _eq_on("A", "Qi", dump["Qi"], rec["Qi"], np.ones(rec["Qi"].shape, bool))
    _eq_on("A", "sQ", dump["sQ"].view(np.int32), rec["sQ"].view(np.int32), np.ones(rec["sQ"].shape, bool))
    return 0


def check_B(dump, rec):
    """m bit-identical on every computed tile."""
    _eq_on("B", "m", np.ascontiguousarray(dump["m"]).view(np.int32), np.ascontiguousarray(rec["m"]).view(np.int32),
           np.broadcast_to(_tile_mask(rec), rec["m"].shape))
    return 0


def check_C(dump, rec):
    """sP within EPS_SP of the restatement's, and exactly the floor where the restatement's is below it; returns
    the largest relative difference."""
    form = rec["form"]
    eps, floor = EPS_SP[form], FLOOR[form]
    on = np.broadcast_to(rec["visited"][None, None], rec["sP"].shape)
    got, want = dump["sP"].astype(np.float64), rec["sP"].astype(np.float64)
    rel = np.abs(got - want) / np.where(on, want, 1.0) * on
    if not (rel <= eps).all():
        i = tuple(int(v) for v in np.argwhere(~(rel <= eps))[0])
        _fail("C", f"sP{list(i)} = {got[i]!r}, restated {want[i]!r}: relative {rel[i]:.3e} > {eps:.3e}")
    floored = on & (rec["sP_raw"].astype(np.float64) < float(floor) * (1.0 - eps))
    _eq_on("C", "sP (floor)", dump["sP"], np.full_like(dump["sP"], floor), floored)
    return float(rel.max())


def near_half(x):
    """Distance of x from the nearest half-integer."""
    return np.abs(x - np.floor(x) - 0.5)


def check_D(dump, rec):
    """Pi equal wherever x is farther than DELTA from a half-integer, off by exactly 1 at most inside; masked
    entries exactly 0; returns (excused entries, computed entries)."""
    el = np.broadcast_to(np.repeat(_tile_mask(rec), GROUP, axis=3), rec["Pi"].shape)
    got, want = dump["Pi"].astype(np.int32), rec["Pi"].astype(np.int32)
    diff = np.where(el, got - want, 0)
    near = near_half(rec["x"]) <= DELTA
    bad = (diff != 0) & ~(near & (np.abs(diff) == 1))
    if bad.any():
        i = tuple(int(v) for v in np.argwhere(bad)[0])
        _fail("D", f"Pi{list(i)} = {got[i]}, restated {want[i]} at x = {rec['x'][i]!r} ({int(bad.sum())} entries)")
    if rec["causal"]:
        B, h, Nq, Nk = got.shape
        masked = el & (np.arange(Nk)[None, :] > np.arange(Nq)[:, None] + (Nk - Nq))
        _eq_on("D", "masked Pi", got, np.zeros_like(got), masked)
    excused, total = int((diff != 0).sum()), int(el.sum())
    if excused > MAX_EXCUSED_SHARE * total:
        _fail("D", f"{excused} of {total} entries differ by 1 near a half-integer: above {MAX_EXCUSED_SHARE}")
    return excused, total


def near_half_share(rec):
    """The share of computed entries whose x lies within DELTA of a half-integer (what D could excuse)."""
    el = np.broadcast_to(np.repeat(_tile_mask(rec), GROUP, axis=3), rec["x"].shape)
    return float((el & (near_half(rec["x"]) <= DELTA)).sum() / el.sum())


def check_E(dump, rec):
    """T == Pi_dump @ Vi in integers, every computed tile."""
    Pi, Vi = dump["Pi"].astype(np.int32), rec["Vi"].astype(np.int32)
    B, h, Nq, Nk = Pi.shape
    Gk = Nk // GROUP
    want = np.einsum("bhqtj,bhtjd->bhtqd", Pi.reshape(B, h, Nq, Gk, GROUP), Vi.reshape(B, h, Gk, GROUP, -1))
    on = np.broadcast_to(_tile_mask(rec).transpose(0, 1, 3, 2)[..., None], want.shape)
    _eq_on("E", "T", dump["T"], want.astype(np.int32), on)
    return 0


def _eps_rows(rec, m, base):
    """[B, h, Nq]: (base + Gk / 2 + 1.5 R) e per row, Gk the row's computed tiles, R its group's re-anchors."""
    gk = np.repeat(rec["visited"].sum(axis=1), GROUP)[None, None]
    return (base + gk / 2.0 + 1.5 * np.repeat(reanchors(m, rec), GROUP, axis=2)) * E_ULP


def check_F(dump, rec):
    """l against the float64 sum of the restatement's p under the dump's own m; returns the largest error / bound."""
    want = l_f64(rec, dump["m"])
    bound = _eps_rows(rec, dump["m"], 7.5) * want + 32.0 * rec["visited"].shape[1] * 2.0 ** -126
    err = np.abs(dump["l"].astype(np.float64) - want)
    if not (err <= bound).all():
        i = tuple(int(v) for v in np.argwhere(~(err <= bound))[0])
        _fail("F", f"l{list(i)} = {dump['l'][i]!r}, float64 sum {want[i]!r}: off by {err[i]:.3e} > {bound[i]:.3e}")
    return float((err / bound).max())


def check_G(dump, rec):
    """O against the float64 replay of the dump's own T, sP, m and l; returns the largest error / bound."""
    want, mag = replay_f64(dump, rec)
    B, h, Nq = dump["l"].shape
    d = want.shape[2] // h
    eps = np.repeat(_eps_rows(rec, dump["m"], 5.0).transpose(0, 2, 1), d, axis=2)  # [B, Nq, h d]
    dead = np.repeat((dump["l"] <= F(1e-20)).transpose(0, 2, 1), d, axis=2)
    O = dump["O"].astype(np.float64)
    if (dead & (dump["O"] != 0)).any():
        _fail("G", "a row with l <= 1e-20 is not exactly 0")
    bound = eps * mag + 1e-30
    err = np.abs(O - want)
    if not (err <= bound).all():
        i = tuple(int(v) for v in np.argwhere(~(err <= bound))[0])
        _fail("G", f"O{list(i)} = {O[i]!r}, replay {want[i]!r}: off by {err[i]:.3e} > {bound[i]:.3e}")
    return float((err / bound).max())


def check_H(dump, rec, sentinel):
    """Tiles that are not computed keep the sentinel; every computed one is written."""
    tile = np.broadcast_to(_tile_mask(rec), rec["m"].shape)
    el = np.repeat(tile, GROUP, axis=3)
    grp = np.broadcast_to(rec["visited"][None, None], rec["sP"].shape)
    tt = np.broadcast_to(_tile_mask(rec).transpose(0, 1, 3, 2)[..., None], rec["T"].shape)
    for name, on in (("S", el), ("m", tile), ("sP", grp), ("Pi", el), ("T", tt)):
        got = dump[name]
        mark = np.asarray(sentinel[name], got.dtype)
        if (~on & (got != mark)).any():
            _fail("H", f"{name}: {int((~on & (got != mark)).sum())} entries of tiles that are not computed were written")
        if (on & (got == mark)).any():
            _fail("H", f"{name}: {int((on & (got == mark)).sum())} entries of computed tiles were not written")
    for name in ("Qi", "sQ", "l"):
        if (dump[name] == np.asarray(sentinel[name], dump[name].dtype)).any():
            _fail("H", f"{name}: entries of active rows were not written")
    return 0


def check_all(dump, rec, sentinel=None):
    """Every check; returns {"C": rel, "D": (excused, total), "F": err / bound, "G": err / bound}."""
    if sentinel is not None:
        check_H(dump, rec, sentinel)
    check_A(dump, rec)
    check_B(dump, rec)
    out = {"C": check_C(dump, rec), "D": check_D(dump, rec)}
    check_E(dump, rec)
    out["F"] = check_F(dump, rec)
    out["G"] = check_G(dump, rec)
    return out


def fill_untouched(dump, rec, sentinel):
    """A synthetic dump as a kernel leaves it: the entries of tiles that are not computed hold the sentinel."""
    tile = np.broadcast_to(_tile_mask(rec), rec["m"].shape)
    el = np.repeat(tile, GROUP, axis=3)
    grp = np.broadcast_to(rec["visited"][None, None], rec["sP"].shape)
    tt = np.broadcast_to(_tile_mask(rec).transpose(0, 1, 3, 2)[..., None], rec["T"].shape)
    for name, on in (("S", el), ("m", tile), ("sP", grp), ("Pi", el), ("T", tt)):
        dump[name] = np.where(on, dump[name], np.asarray(sentinel[name], dump[name].dtype))
    return dump
