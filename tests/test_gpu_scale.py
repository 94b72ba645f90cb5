"""GPU tests (MI355X) of the masked kernel family (qmha_fa_masked.hip: SquareCausal, Rect, Grouped, Varlen) at the
scale it is measured and advertised at: wide ragged grids, 128-tile key loops, more workgroups than the
device holds at once, and independence of whatever the previous launch left behind.

Bit-identity with narrow calls does most of the work and costs nothing on the CPU:
  1. one wide call is compared, slice by slice -- ALL slices -- with B = 1, h = 1 (grouped: h_kv = 1) calls of the same
     entry point on the slice's columns.  The narrow call runs the same template instance on 1 - 5 workgroups, the
     regime the other suites hold to the CPU restatements, so a wrong bh, pair index, unit or column offset in the wide
     launch moves whole tiles.  Two slices of the square and rect causal calls are also held to the restatements
     themselves, so the block does not rest on two GPU paths agreeing;
  2. qmha_solve_rect at Nk = 4096 (128 tiles in one wave) is held to tests/rect_ref.py at the rectangular suite's
     bounds, and the K/V cache, the grouped cache, attend_varlen and the square causal call hang on it bit for bit;
  3. B16 h16 N2048 square causal -- 2048 (int8) / 4096 (fp16) workgroups, at least 1.5 x what the device holds -- is
     compared on eight slices with narrow calls, range-checked everywhere and held to float64 on 96 rows of two slices;
  4. a clean call, the same call on K / V of +-1e30 with NaNs, and the clean call again give the same bits twice.
tests/test_scale_cpu.py holds the shapes and asserts, from the kernels' launch formulas, that each reaches its case.
Every O is the head of a buffer with a sentinel-filled guard behind it.  Every bound is one the project already uses:
2 u_r + 5e-5, fp16_lazy_tol, verify_results(1e-3, 1e-3), the 5e-3 int8 budget against float64, or exact equality.
"""
import functools

import numpy as np
import pytest

from tests import causal_ref as cr
from tests import parity_log
from tests import rect_ref as rr
from tests import test_scale_cpu as sc
from tests.gpu_support import (BUILT, F16, INT8, Guarded, assert_bits, assert_f16, assert_int8, assert_zeros, attend,
                               dev, i32, new_cache, seq_slices, to_dev)  # noqa: F401

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
TAG = "+s"  # this file's mark on its parity_log records
_vd = lambda v: "-".join(str(x) for x in v) if isinstance(v, tuple) else str(v)  # noqa: E731


def cols(X, k, w):
    """Columns [k w, (k + 1) w) of a device tensor, contiguous."""
    return X[..., k * w:(k + 1) * w].contiguous()


def solve(variant, t, h, causal, h_kv=None, device_result=False):
    """flash_solve (square causal: qmha_solve_opts), flash_solve_rect or flash_solve_gqa on device tensors t."""
    from quantizedmha_amd import torch_ext
    Q, K, V = t
    g = Guarded(Q)
    if h_kv is not None:
        torch_ext.flash_solve_gqa(Q, K, V, Q.shape[-1], h, h_kv, variant, out=g.out, causal=causal)
    elif causal and Q.shape == K.shape:
        torch_ext.flash_solve(Q, K, V, Q.shape[-1], h, variant, out=g.out, causal=True)
    else:
        torch_ext.flash_solve_rect(Q, K, V, Q.shape[-1], h, variant, out=g.out, causal=causal)
    return g.device_result() if device_result else g.result()


# ==== 1. the launch map on ragged, wide grids ============================================================================
_WIDE = {}


def wide(dev, name, variant, d, causal=True, entry="solve"):
    """(device inputs, O of the wide call), computed once per case and left unchanged."""
    key = (name, variant, d, causal, entry)
    if key not in _WIDE:
        w = sc.WIDE[name]
        t = to_dev(dev, *sc.wide_inputs(name, d))
        if entry == "solve":
            got = solve(variant, t, w.h, causal, h_kv=w.h_kv if w.h_kv != w.h else None)
        else:  # the grouped cache, full: attend at len == cap
            cache = new_cache(dev, variant, w.B, w.Nk, d, w.h, w.h_kv)
            cache.append(t[1], t[2])
            got = attend(cache, t[0], causal)
        _WIDE[key] = (t, got)
    return _WIDE[key]


@pytest.mark.parametrize("name,causal", [("square", True), ("rect", True), ("rect", False)], ids=_vd)
@pytest.mark.parametrize("variant,d", BUILT)
def test_wide_multi_head_call_equals_its_narrow_calls(dev, variant, d, name, causal):
    """B3 h5, N640 square causal (int8 45 / fp16 75 workgroups; nqb = 5: an unpaired middle block) and Nq416 Nk640
    rectangular (30 / 60; 13 query groups: the last unit block has one active wave; diag_off 7), causal and unmasked:
    every (b, k) against the B = 1, h = 1 call on that slice's columns, bit for bit."""
    w = sc.WIDE[name]
    (Q, K, V), got = wide(dev, name, variant, d, causal)
    assert np.isfinite(got).all()
    for b in range(w.B):
        for k in range(w.h):
            one = solve(variant, [cols(x[b:b + 1], k, d) for x in (Q, K, V)], 1, causal)
            assert_bits(f"{name} slice ({b}, {k})", got[b:b + 1, :, k * d:(k + 1) * d], one)
    assert len({got[b, :, k * d:(k + 1) * d].tobytes() for b in range(w.B) for k in range(w.h)}) == w.B * w.h


@pytest.mark.parametrize("entry", ["solve", "cache"])
@pytest.mark.parametrize("variant,d", BUILT)
def test_wide_grouped_call_equals_its_narrow_calls(dev, variant, d, entry):
    """B3 h9 h_kv3 (G = 3) Nq160 Nk288 causal, qmha_solve_gqa and GroupedKVCache.attend (18 / 36 workgroups; 15 units:
    a unit block mixes query groups and heads): every (b, kvh) against the B = 1, h_kv = 1 call with its G query heads."""
    w = sc.WIDE["grouped"]
    G = w.h // w.h_kv
    (Q, K, V), got = wide(dev, "grouped", variant, d, True, entry)
    for b in range(w.B):
        for kvh in range(w.h_kv):
            q, k, v = cols(Q[b:b + 1], kvh, G * d), cols(K[b:b + 1], kvh, d), cols(V[b:b + 1], kvh, d)
            if entry == "solve":
                one = solve(variant, [q, k, v], G, True, h_kv=1)
            else:
                cache = new_cache(dev, variant, 1, w.Nk, d, G, 1)
                cache.append(k, v)
                one = attend(cache, q, True)
            assert_bits(f"grouped {entry} slice ({b}, {kvh})", got[b:b + 1, :, kvh * G * d:(kvh + 1) * G * d], one)


@pytest.mark.parametrize("causal", [True, False], ids=["causal", "full"])
@pytest.mark.parametrize("variant,d", BUILT)
def test_wide_varlen_call_equals_uniform_narrow_caches(dev, variant, d, causal):
    """B7 h6 h_kv3 (G = 2) Nq96 cap288, lens [288, 96, 0, 192, 100, 288, 128] (21 / 42 workgroups): sequences 2 and 4
    are positive zeros; every other (b, kvh) equals the uniform attend of a B = 1, h_kv = 1 cache holding lens[b] rows
    -- causal: of capacity 288; unmasked: a full cache of cap = lens[b]."""
    w = sc.WIDE["varlen"]
    G = w.h // w.h_kv
    Q, K, V = to_dev(dev, *sc.wide_inputs("varlen", d))
    cache = new_cache(dev, variant, w.B, w.Nk, d, w.h, w.h_kv)
    cache.append(K, V)
    got = attend(cache, Q, causal, lens=i32(dev, sc.VARLEN_LENS))
    for b, L in enumerate(sc.VARLEN_LENS):
        if not sc.varlen_valid(L, w.Nq, w.Nk, causal):
            assert_zeros(f"sequence {b} (lens = {L})", got[b])
            continue
        for kvh in range(w.h_kv):
            one = new_cache(dev, variant, 1, w.Nk if causal else L, d, G, 1)
            one.append(cols(K[b:b + 1, :L], kvh, d), cols(V[b:b + 1, :L], kvh, d))
            want = attend(one, cols(Q[b:b + 1], kvh, G * d), causal)
            assert_bits(f"varlen slice ({b}, {kvh}) at {L}", got[b:b + 1, :, kvh * G * d:(kvh + 1) * G * d], want)


@pytest.mark.parametrize("variant,d", BUILT)
def test_wide_append_at_places_what_narrow_appends_place(dev, variant, d):
    """append_at(n = 64, pos = [0, 64, -32, 128, 48, 160, 224]) on the B7 grouped cache, prefilled with a byte pattern:
    sequence b's bytes are those of a B = 1 cache holding the same pattern and appended at len == pos[b]; sequences 2
    and 4 (negative, no multiple of 32) and everything else keep the pattern."""
    w = sc.WIDE["varlen"]
    n = sc.VARLEN_N
    _, K, V = to_dev(dev, *sc.wide_inputs("varlen", d))
    new_k, new_v = K[:, 96:96 + n].contiguous(), V[:, 96:96 + n].contiguous()
    a = new_cache(dev, variant, w.B, w.Nk, d, w.h, w.h_kv)
    pattern = (torch.arange(a.mem.numel(), device=dev) % 251).to(torch.uint8)
    a.mem.copy_(pattern)
    a.append_at(new_k, new_v, i32(dev, sc.VARLEN_POS))
    want = pattern.clone()
    for b, p in enumerate(sc.VARLEN_POS):
        if not (p >= 0 and p % 32 == 0):
            continue
        u = new_cache(dev, variant, 1, w.Nk, d, w.h, w.h_kv)
        if p:
            u.append(K[b:b + 1, :p], V[b:b + 1, :p])  # only to move len to pos[b]
        mine, theirs = seq_slices(a, b), seq_slices(u, 0)
        for sa, su in zip(mine, theirs):
            u.mem[su] = pattern[sa]
        u.append(new_k[b:b + 1], new_v[b:b + 1])
        for sa, su in zip(mine, theirs):
            want[sa] = u.mem[su]
    torch.cuda.synchronize()
    changed = [bool((want[s] != pattern[s]).any()) for b in range(w.B) for s in seq_slices(a, b)[:1]]
    assert changed == [True, True, False, True, False, True, True]
    assert torch.equal(a.mem, want)


@functools.lru_cache(maxsize=None)
def wide_reference(name, variant, b, k):
    """Restatement (and, fp16, float64) of slice (b, k) of the causal wide call at d = 64, computed once."""
    from oracle import oracle
    q, kk, v = (sc.head_cols(x[b:b + 1], k, 64) for x in sc.wide_inputs(name, 64))
    if variant == INT8:
        ref, unit = rr.fa_int8(oracle, q, kk, v, 64, 1, causal=True, base2=True)
        return ref, cr.per_element(unit, 64)
    return rr.fa_fp16_lazy(None, q, kk, v, 64, 1, causal=True), rr.attention_f64(q, kk, v, 64, 1, True)


@pytest.mark.parametrize("name", ["square", "rect"])
@pytest.mark.parametrize("variant", [INT8, F16])
def test_wide_causal_calls_vs_the_restatements(dev, variant, name):
    """The independent anchor of this block: slices (0, 0) and (2, 4) of the square and the rectangular causal wide
    calls at d = 64 against rect_ref, at tests/test_gpu_rect.py's bounds."""
    w = sc.WIDE[name]
    _, got = wide(dev, name, variant, 64, True)
    for b, k in sc.ANCHOR_SLICES:
        mine = np.ascontiguousarray(got[b:b + 1, :, k * 64:(k + 1) * 64])
        label = f"wide {name} B{w.B} h{w.h} slice ({b}, {k})"
        if variant == INT8:
            assert_int8(label, mine, *wide_reference(name, variant, b, k), TAG)
        else:
            contract, exact = wide_reference(name, variant, b, k)
            assert_f16(label, mine, contract, cr.fp16_lazy_tol(w.Nk), TAG, exact)


# ==== 2. long key loops: 128 tiles =========================================================================================
_LONG_DEV, _LONG = {}, {}


def long_dev(dev, d, dist):
    """Device Q [1, 256, 2 d], K, V [1, 4096, 2 d]."""
    if (d, dist) not in _LONG_DEV:
        _LONG_DEV[(d, dist)] = to_dev(dev, *sc.long_inputs(d, dist))
    return _LONG_DEV[(d, dist)]


def long_base(dev, variant, d, dist, call):
    """O of qmha_solve_rect, B = 1, h = 2, Nk = 4096, for one of sc.LONG_CALLS; computed once and left unchanged."""
    key = (variant, d, dist, call)
    if key not in _LONG:
        _, Nq, causal = call
        Q, K, V = long_dev(dev, d, dist)
        _LONG[key] = solve(variant, [Q[:, 256 - Nq:].contiguous(), K, V], sc.LONG_H, causal)
    return _LONG[key]


@pytest.mark.parametrize("call", sc.LONG_CALLS, ids=lambda c: c[0])
@pytest.mark.parametrize("dist", rr.DISTS)
@pytest.mark.parametrize("d", [32, 64, 128])
def test_long_int8_vs_base2_restatement(dev, d, dist, call):
    """Nk = 4096: every element within 2 u_r + 5e-5 of rect_ref.fa_int8(base2=True), and (rows >= 32 of the causal
    calls are all of them: the queries are the last rows of 4096) within the 5e-3 int8 budget of float64."""
    _, Nq, causal = call
    ref, unit, exact = sc.long_int8_reference(d, dist, causal)
    got = long_base(dev, INT8, d, dist, call)
    assert_int8(f"Nk4096 {call[0]} d{d} {dist}", got, ref[:, -Nq:], unit[:, -Nq:], TAG)
    far = float(np.abs(got - exact[:, -Nq:]).max())
    print(f"Nk4096 {call[0]} d{d} {dist}: max|gpu - float64| = {far:.3e} (bound 5e-3)")
    assert far <= 5e-3, far


@pytest.mark.parametrize("call", sc.LONG_CALLS, ids=lambda c: c[0])
@pytest.mark.parametrize("dist", rr.DISTS)
@pytest.mark.parametrize("d", [64, 128])
def test_long_fp16_vs_lazy_contract_and_float64(dev, d, dist, call):
    """Nk = 4096: head 0 within fp16_lazy_tol(4096) of rect_ref.fa_fp16_lazy (one head: the restatement costs 4 - 12 s a
    head at this length), both heads within max(1e-3, 1e-3 |ref|) of float64."""
    _, Nq, causal = call
    contract, exact = sc.long_f16_reference(d, dist, causal)
    got = long_base(dev, F16, d, dist, call)
    assert_f16(f"Nk4096 {call[0]} d{d} {dist}", np.ascontiguousarray(got[..., :d]), contract[:, -Nq:],
               cr.fp16_lazy_tol(sc.LONG_NK), TAG, exact[:, -Nq:], got_all=got)


@pytest.mark.parametrize("call", sc.LONG_CALLS, ids=lambda c: c[0])
@pytest.mark.parametrize("variant,d", BUILT)
def test_long_family_equals_the_rect_call(dev, variant, d, call):
    """The rest of the family on the base call, bit for bit: KVCache filled by appends of 1024 + 3072 rows; a
    GroupedKVCache with G = 4 whose four query heads per K/V head repeat the base call's head (four active waves where
    the base call has one); attend_varlen with lens = [4096] in a cache of cap 4096; attend_varlen with lens
    [2080, 4096] in a cache of cap 4128 (B = 2) against qmha_solve_rect at Nk = 2080 and the base call."""
    _, Nq, causal = call
    h = sc.LONG_H
    Q, K, V = long_dev(dev, d, "normal")
    q = Q[:, 256 - Nq:].contiguous()
    base = long_base(dev, variant, d, "normal", call)
    cache = new_cache(dev, variant, 1, sc.LONG_NK, d, h)
    cache.append(K[:, :1024], V[:, :1024])
    cache.append(K[:, 1024:], V[:, 1024:])
    assert cache.len == sc.LONG_NK
    assert_bits("KVCache 1024 + 3072", attend(cache, q, causal), base)
    assert_bits("attend_varlen [4096]", attend(cache, q, causal, lens=i32(dev, [sc.LONG_NK])), base)
    G = 4
    grouped = new_cache(dev, variant, 1, sc.LONG_NK, d, G * h, h)
    grouped.append(K, V)
    q4 = q.view(1, Nq, h, 1, d).expand(1, Nq, h, G, d).reshape(1, Nq, G * h * d).contiguous()
    got = attend(grouped, q4, causal).reshape(1, Nq, h, G, d)
    for j in range(G):
        assert_bits(f"GroupedKVCache G = 4, query head j = {j}", got[:, :, :, j].reshape(1, Nq, h * d), base)
    lens, cap = sc.LONG_VARLEN
    k2, v2 = (torch.full((2, cap, h * d), 1e30 * s, dtype=torch.float32, device=dev) for s in (1, -1))
    for b, L in enumerate(lens):
        k2[b, :L], v2[b, :L] = K[0, :L], V[0, :L]
    two = new_cache(dev, variant, 2, cap, d, h)
    two.append(k2, v2)
    got = attend(two, torch.cat([q, q]), causal, lens=i32(dev, lens))
    short = solve(variant, [q, K[:, :lens[0]].contiguous(), V[:, :lens[0]].contiguous()], h, causal)
    assert_bits(f"attend_varlen, sequence 0 at {lens[0]}", got[:1], short)
    assert_bits(f"attend_varlen, sequence 1 at {lens[1]}", got[1:], base)
    assert not np.array_equal(short, base)


@pytest.mark.parametrize("variant", [INT8, F16])
def test_long_square_causal_call_ends_in_the_rect_call(dev, variant):
    """Square causal N = 4096, h = 1, d = 64 (the SquareCausal instance over 128 tiles): its last 256 rows equal the
    Nq = 256 rectangular call on the same K / V, which is head 0 of the base call."""
    d = 64
    Q, K, V = long_dev(dev, d, "normal")
    k, v = cols(K, 0, d), cols(V, 0, d)
    gen = torch.Generator(device=dev).manual_seed(4096)
    q = torch.randn((1, sc.LONG_NK, d), generator=gen, device=dev) * 0.5
    q[:, -256:] = cols(Q, 0, d)
    rect = solve(variant, [cols(Q, 0, d), k, v], 1, True)
    assert_bits("h = 1 rect call against head 0 of the base call", rect, long_base(dev, variant, d, "normal", sc.LONG_CALLS[0])[..., :d])
    square = solve(variant, [q, k, v], 1, True)
    assert np.isfinite(square).all()
    assert_bits("last 256 rows of the square causal call", square[:, -256:], rect)


# ==== 3. more workgroups than the device holds ==============================================================================
def rows_f64(Q, K, V, r0, r1):
    """float64 causal attention of rows [r0, r1) of one square slice [N, d]: bottom-right aligned over keys [0, r1)."""
    return rr.attention_f64(Q[r0:r1], K[:r1], V[:r1], Q.shape[-1], 1, causal=True)


@pytest.mark.parametrize("variant", [INT8, F16])
def test_more_workgroups_than_the_device_holds(dev, variant):
    """Square causal B16 h16 N2048 d64: 2048 (int8, nqb 16, 8 pairs) / 4096 (fp16) workgroups, at least 1.5 x the
    resident capacity (tests/test_scale_cpu.py), so later workgroups start on compute units, LDS and registers that
    earlier ones of the same launch have just left.  Eight slices -- the first, the last, six launched in the last
    third of the grid -- equal their B = 1, h = 1 calls bit for bit; all of O is finite and per head within
    [min V - 1e-4, max V + 1e-4]; rows 32..63, 1024..1055 and 2016..2047 of two slices are held to float64 causal
    attention (int8: 5e-3; fp16: max(1e-3, 1e-3 |ref|); rows < 32 carry V's quantisation step).
    The rectangular shape B16 h16 Nq512 Nk2048 (512 / 1024 workgroups) does not exceed capacity by 1.5 x and is left out.
    Inputs are N(0, 0.25) drawn on the device, with rows 0..31 of V halved.  That is what makes the range check a
    property of the contract: a row that attends a handful of keys is a few rows of V as the kernel holds them -- half
    or int8 V under half or int8 p, each a rounding of up to 1e-3 at |V| = 2 -- so where a head's extreme value of V
    stands in row 0, O[0] legitimately passes it (measured with unscaled V: fp16 (b 8, head 15) row 0, O = -2.21313
    under min V = -2.21247, the slice bit-identical to its narrow call).  With the early rows of V at half size every
    row of O is a near-convex mix of values at least 1 inside the head's range, or of 33 and more keys."""
    from oracle import oracle
    o, d = sc.OVER_SQUARE, 64
    gen = torch.Generator(device=dev).manual_seed(2048 + len(variant))
    Q, K, V = (torch.randn((o.B, o.Nq, o.h * d), generator=gen, device=dev) * 0.5 for _ in range(3))
    V[:, :32] *= 0.5
    got = solve(variant, [Q, K, V], o.h, True, device_result=True)
    assert bool(torch.isfinite(got).all())
    o4, v4 = got.view(o.B, o.Nq, o.h, d), V.view(o.B, o.Nq, o.h, d)
    assert bool((o4.amin(dim=(1, 3)) >= v4.amin(dim=(1, 3)) - 1e-4).all()) and bool((o4.amax(dim=(1, 3)) <= v4.amax(dim=(1, 3)) + 1e-4).all())
    for n, (b, k) in enumerate(sc.OVER_SLICES):
        t = [cols(x[b:b + 1], k, d) for x in (Q, K, V)]
        mine = cols(got[b:b + 1], k, d).cpu().numpy()
        assert_bits(f"slice ({b}, {k})", mine, solve(variant, t, 1, True))
        if n in (1, 4):  # (15, 15) and (5, 15)
            q, kk, v = (x[0].cpu().numpy() for x in t)
            for r0 in (32, 1024, 2016):
                exact = rows_f64(q, kk, v, r0, r0 + 32)
                far = float(np.abs(mine[0, r0:r0 + 32] - exact).max())
                print(f"{variant} B16 h16 N2048 slice ({b}, {k}) rows {r0}..{r0 + 31}: max|gpu - float64| = {far:.3e}")
                parity_log.record(f"B16 h16 N2048 slice ({b}, {k}) rows {r0}.. (vs float64)", variant + TAG, far, 0.0,
                                  5e-3 if variant == INT8 else 1e-3)
                if variant == INT8:
                    assert far <= 5e-3, far
                else:
                    assert oracle.verify_results(np.ascontiguousarray(mine[0, r0:r0 + 32]), exact.astype(np.float32), 1e-3, 1e-3) == -1, far


# ==== 4. results do not depend on what ran before ===========================================================================
def poisoned(X, sign):
    """Magnitude 1e30 (fp16: inf in the staged tiles; int8: saturated operands and huge scales), a NaN in every
    32-row group: values the suites already feed these kernels."""
    P = torch.full_like(X, sign * 1e30)
    P[:, 5::32, 3::16] = float("nan")
    return P


@pytest.mark.parametrize("Nq,Nk,causal", sc.AFTER_SHAPES)
@pytest.mark.parametrize("variant,d", BUILT)
def test_result_does_not_depend_on_the_previous_launch(dev, variant, d, Nq, Nk, causal):
    """A probe, not a proof: the clean call, the same call on poisoned K / V, and the clean call again are enqueued back
    to back on one stream; the two clean results must be bit-identical.  Nothing forces the third launch onto the
    compute units the second used, though on grids this small (4 - 8 workgroups) it usually lands there; what the
    second left in LDS and registers is then what the third starts on.  Of the poisoned O only the guard is checked."""
    from quantizedmha_amd import torch_ext
    B, h = 2, 2
    Q, K, V = to_dev(dev, *rr.inputs(Nq, Nk, h * d, B, "normal", 8800 + Nq + d))
    runs = [(K, V), (poisoned(K, 1.0), poisoned(V, -1.0)), (K, V)]
    outs = [Guarded(Q) for _ in runs]
    for g, (k, v) in zip(outs, runs):
        torch_ext.flash_solve_rect(Q, k, v, h * d, h, variant, out=g.out, causal=causal)
    first, _, again = [g.result() for g in outs]
    assert np.isfinite(first).all() and np.abs(first).max() > 0.0
    assert_bits("the clean call after the poisoned one", again, first)


@pytest.mark.parametrize("Nq,Nk,causal", sc.AFTER_SHAPES)
@pytest.mark.parametrize("variant,d", BUILT)
def test_varlen_result_does_not_depend_on_the_previous_launch(dev, variant, d, Nq, Nk, causal):
    """The same probe through GroupedKVCache.attend_varlen (h = 4 on h_kv = 2, lens = [Nk, Nk]): a clean cache, a
    poisoned cache of the same geometry, the clean cache again."""
    B, h, h_kv = 2, 4, 2
    Q = to_dev(dev, rr.inputs(Nq, Nk, h * d, B, "normal", 8900 + Nq + d)[0])[0]
    K, V = to_dev(dev, *rr.inputs(Nq, Nk, h_kv * d, B, "normal", 8901 + Nq + d)[1:])
    clean, dirty = (new_cache(dev, variant, B, Nk, d, h, h_kv) for _ in range(2))
    clean.append(K, V)
    dirty.append(poisoned(K, 1.0), poisoned(V, -1.0))
    lens = i32(dev, [Nk, Nk])
    outs = [Guarded(Q) for _ in range(3)]
    for g, cache in zip(outs, (clean, dirty, clean)):
        cache.attend_varlen(Q, lens, causal=causal, out=g.buf[:g.n])
    first, _, again = [g.result() for g in outs]
    assert np.isfinite(first).all() and np.abs(first).max() > 0.0
    assert_bits("the clean cache after the poisoned one", again, first)
    assert_bits("attend_varlen against attend", first, attend(clean, Q, causal))
