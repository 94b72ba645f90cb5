"""GPU tests of the e4m3 K/V cache kernels on hard numerics and multi-stage chunks: the appends on the e4m3
edge table, byte for byte; the attends on the score families of tests/fp8_hard.py against the restatements, within FLIPS
one-flip units u = 2^-4 * 2^8 * max|v| / l plus 2^-16 max|V| (FLIPS = 2), O and every partial the combine
reads; the decode kernels' stage loop at chunk_rows 192 ... 768 and pools of 64 ... 384-row pages at cap 768.  What the
families reach, and that the comparison used here fails on a subtly wrong kernel, is tests/test_fp8_hard_cpu.py's."""
import functools

import numpy as np
import pytest
import torch

from tests import decode_ref, fp8_ref
from tests import decode_window_ref as dwr
from tests import fp8_hard as H
from tests.gpu_support import Guarded, assert_bits, dev, i32  # noqa: F401

pytestmark = pytest.mark.gpu
FP8, FILL, B, CAP = "fa_tc_fp8", 0x5A, H.B, H.CAP
FAMILY = pytest.mark.parametrize("name", H.FAMILIES)
EACH_D = pytest.mark.parametrize("d", [64, 128])


@functools.lru_cache(maxsize=None)
def table_of(nb, max_pages):
    """A permuted block table over nb max_pages + 1 pages: the last page of the permutation is in no sequence."""
    return np.random.default_rng(max_pages).permutation(nb * max_pages + 1)[:-1].reshape(nb, max_pages).astype(np.int32)


def new_cache(dev, nb, cap, d, h, hk, scales, page_rows=None, fill=0):
    """(cache, table): a contiguous cache, or a pool of page_rows-row pages under table_of; every byte `fill`."""
    from quantizedmha_amd import torch_ext
    if page_rows is None:
        cache, table = torch_ext.GroupedKVCache(nb, cap, h * d, h, hk, FP8, str(dev)), None
    else:
        mp = -(-cap // page_rows)  # cap 224: four 64-row pages a sequence
        cache = torch_ext.PagedKVCache(nb, nb * mp + 1, page_rows, mp, h * d, h, hk, FP8, str(dev))
        table = i32(dev, table_of(nb, mp).tolist())
    cache.mem.fill_(fill), cache.set_scales(*scales), cache.enable_tokens()
    return cache, table


def fill(cache, table, K, V, rows=None):
    """Rows [0, rows[b]) of every sequence (default: all of K) in one append per distinct count."""
    nb, cap = K.shape[:2]
    rows = [cap] * nb if rows is None else rows
    for n in sorted(set(rows)):
        Kn, Vn = (torch.from_numpy(np.ascontiguousarray(x[:, :n])).to(cache.mem.device) for x in (K, V))
        pos = i32(cache.mem.device, [0 if r == n else -1 for r in rows])
        cache.append_tokens(Kn, Vn, pos) if table is None else cache.append_paged(Kn, Vn, pos, table)
    return cache, table


def full_cache(dev, K, V, d, h, hk, scales=H.SCALES, page_rows=None, fill_byte=0):
    return fill(*new_cache(dev, K.shape[0], K.shape[1], d, h, hk, scales, page_rows, fill_byte), K, V)


def prefill(cache, table, Q, lens):
    g = Guarded(Q)
    (cache.attend_tokens if table is None else cache.attend_paged)(Q, i32(Q.device, lens), *([] if table is None else [table]), out=g.buf[:g.n])
    return g.result()


def decode(cache, table, Q, lens, chunk, window=None, sinks=None, guard=0):
    """O through the guard and the scratch (float32) of a decode call over a NaN-filled scratch with `guard` bytes behind it."""
    nq, g = Q.shape[1], Guarded(Q)
    if window is None:
        cache.enable_decode(chunk, nq)
        n = cache.decode_scratch.numel()
        cache.decode_scratch = torch.full((n + guard,), 0xFF, dtype=torch.uint8, device=Q.device)
        (cache.attend_decode if table is None else cache.attend_paged_decode)(Q, i32(Q.device, lens), *([] if table is None else [table]), out=g.buf[:g.n])
        scratch = cache.decode_scratch
    else:
        cache.enable_decode_window(chunk, window, nq)
        n = cache.decode_window_scratch.numel()
        cache.decode_window_scratch = torch.full((n + guard,), 0xFF, dtype=torch.uint8, device=Q.device)
        s = None if sinks is None else torch.from_numpy(np.ascontiguousarray(sinks, np.float32)).to(Q.device)
        (cache.attend_decode_window if table is None else cache.attend_paged_decode_window)(Q, i32(Q.device, lens), *([] if table is None else [table]), window, s, out=g.buf[:g.n])
        scratch = cache.decode_window_scratch
    out = g.result()
    scratch = scratch.cpu().numpy()
    assert (scratch[n:] == 0xFF).all(), "written behind the scratch"
    return out, scratch[:n].view(np.float32)


def hold(label, got, scratch, want, d, h, V):
    """O and every partial the combine reads within the bound of the restatement `want`; finite wherever written; the NaN
    pattern of the scratch the restatement's.  Returns the worst err / bound of O and of the partials."""
    O, (Oc, pm, pl), Ltot, vmax = want
    fp32 = H.fp32_term(V, H.SCALES)
    wo = H.compare(label + ": O", got, O, H.o_bound(vmax, Ltot, d, fp32))
    nb, NC, nq, _ = pl.shape
    gOc, gm, gl = decode_ref.views(scratch, nb, NC, nq, h, d)
    assert np.array_equal(np.isnan(gl), np.isnan(pl)) and np.array_equal(np.isnan(gOc), np.isnan(Oc)) and np.array_equal(np.isnan(gm), np.isnan(pm)), label
    assert np.isnan(scratch[decode_ref.layout(nb, NC, nq, h, d)[1] // 4:]).all(), (label, "behind the call's layout")
    w = ~np.isnan(pl)
    if not w.any():
        return wo, 0.0
    wd = np.repeat(w, d, axis=-1)
    assert np.isfinite(gm[w]).all() and np.isfinite(gl[w]).all() and np.array_equal(gl[w] == 0, pl[w] == 0), label
    return wo, H.compare(label + ": partials", gOc[wd], Oc[wd], H.o_bound(vmax, np.where(w & (pl > 0), pl, 1.0), d, fp32)[wd])


# ---- a. the encoding -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def table_kv(d, hk, scales):
    """K, V [B, CAP, hk d]: the edge table times the scale in fp32, rolled by another amount per row, sequence and tensor."""
    t = H.edge_table()
    return tuple(np.stack([(H.place(t, CAP, hk * d, off + 101 * b) * np.float32(s)).astype(np.float32) for b in range(B)])
                 for off, s in ((0, scales[1]), (517, scales[2])))


def expected_mem(nbytes, K, V, rows, scales, d, hk, slice_rows, slices, where):
    """cache.mem: the restatement's bytes in the groups below ceil32(rows[b]), the sentinel elsewhere; where(b, g) -> (slice of
    K/V head 0, group in it)."""
    exp, vo = np.full(nbytes, FILL, np.uint8), slices * slice_rows * d
    assert nbytes == 2 * vo
    for b, L in enumerate(rows):
        for kh in range(hk):
            k8, vt, _ = fp8_ref.cache_arrays(K[b][:, kh * d:(kh + 1) * d], V[b][:, kh * d:(kh + 1) * d], L, scales[1], scales[2])
            for g in range(len(k8) // 32):
                sl, gp = where(b, g)
                at = ((sl + kh) * slice_rows + 32 * gp) * d
                exp[at:at + 32 * d], exp[vo + at:vo + at + 32 * d] = k8[32 * g:32 * g + 32].ravel(), vt[32 * g * d:32 * (g + 1) * d]
    return exp


@pytest.mark.parametrize("scales", [H.UNIT, H.SCALES])
@pytest.mark.parametrize("entry", ["append", "append_at", "append_tokens", "append_paged"])
@EACH_D
def test_edge_table_bytes(dev, d, entry, scales):
    """Every e4m3 edge value through every append entry point: cache.mem byte for byte over a sentinel."""
    hk, (K, V) = 2, table_kv(d, 2, scales)
    Kd, Vd = (torch.from_numpy(x).to(dev) for x in (K, V))
    if entry in ("append", "append_at"):  # whole groups: cap 256, rows 224 .. 255 keep the sentinel
        cache, _ = new_cache(dev, B, 256, d, hk, hk, scales, fill=FILL)
        for lo, hi in ((0, 96), (96, 224)):
            Kn, Vn = Kd[:, lo:hi].contiguous(), Vd[:, lo:hi].contiguous()
            cache.append(Kn, Vn) if entry == "append" else cache.append_at(Kn, Vn, i32(dev, [lo] * B))
        rows, want = (224,) * B, lambda n: expected_mem(n, K, V, (224,) * B, scales, d, hk, 256, B * hk, lambda b, g: (b * hk, g))  # noqa: E731
    else:  # pieces that start at p = 0 and inside a group: a V^T dword is read, merged and stored back
        rows, paged = (224, 100, 33), entry == "append_paged"
        cache, table = new_cache(dev, B, CAP, d, hk, hk, scales, 64 if paged else None, fill=FILL)
        for b, L in enumerate(rows):
            p = 0
            for n in (17, 1, 46, 3, 61, 64, 32):
                n = min(n, L - p)
                if n > 0:
                    Kn, Vn = (x[b:b + 1, p:p + n].expand(B, n, hk * d).contiguous() for x in (Kd, Vd))
                    pos = i32(dev, [p if i == b else -1 for i in range(B)])
                    cache.append_paged(Kn, Vn, pos, table) if paged else cache.append_tokens(Kn, Vn, pos)
                    p += n
        T = table_of(B, 4)
        where = (lambda b, g: (int(T[b][g // 2]) * hk, g % 2)) if paged else (lambda b, g: (b * hk, g))
        want = lambda n: expected_mem(n, K, V, rows, scales, d, hk, 64 if paged else CAP, (B * 4 + 1 if paged else B) * hk, where)  # noqa: E731
    got = cache.mem.cpu().numpy()
    exp = want(got.size)
    assert np.array_equal(got, exp), (int((got != exp).sum()), np.flatnonzero(got != exp)[:8])
    assert (exp == 0x7E).sum() > 0 and (exp == 0xFE).sum() > 0 and not (exp[exp != FILL] & 0x7F == 0x7F).any()


@pytest.mark.parametrize("q_scale", [1.0, 0.5])
@EACH_D
def test_query_encoding_is_idempotent(dev, d, q_scale):
    """Q is the edge table (no inf) times q_scale; attend(Q) and attend(decode(encode(Q)) q_scale) give the same bits."""
    (h, hk, nq), lens, scales = H.HEADS[1], H.lens_of(5, "mid"), (q_scale, 0.7, 1.9)
    _, K, V = H.family("normal", d, h, hk, nq, lens)
    t = H.edge_table(inf=False)
    Q = np.stack([(t[(np.arange(nq * h * d).reshape(nq, h * d) + 211 * b) % len(t)] * np.float32(q_scale)).astype(np.float32) for b in range(B)])
    assert nq * h * d >= len(t)  # every value, in every sequence
    Q2 = np.stack([fp8_ref.decode(fp8_ref.encode(q, q_scale)) * np.float32(q_scale) for q in Q]).astype(np.float32)
    assert not np.array_equal(Q, Q2)
    cache, _ = full_cache(dev, K, V, d, h, hk, scales)
    Qd, Q2d = torch.from_numpy(Q).to(dev), torch.from_numpy(Q2).to(dev)
    for label, call in (("attend_tokens", lambda q: prefill(cache, None, q, lens)), ("attend_decode", lambda q: decode(cache, None, q, lens, 64)[0]),
                        ("attend_decode_window", lambda q: decode(cache, None, q, lens, 128, 33, H.ramp(h))[0]),
                        ("attend_decode_window, combine", lambda q: decode(cache, None, q, lens, 64, 100, H.ramp(h))[0])):
        assert_bits(label, call(Qd), call(Q2d))


# ---- b. the score families at B = 3, cap 224 -----------------------------------------------------------------------------
@FAMILY
@EACH_D
def test_family_prefill(dev, d, name):
    h = hk = 2
    for nq, lens in H.PREFILL:
        Q, K, V = H.family(name, d, h, hk, nq, lens)
        Qd = torch.from_numpy(Q).to(dev)
        got = prefill(*full_cache(dev, K, V, d, h, hk), Qd, lens)
        assert_bits("paged against contiguous", prefill(*full_cache(dev, K, V, d, h, hk, page_rows=64), Qd, lens), got)
        ref, bound = np.zeros(Q.shape), np.zeros(Q.shape)
        for b, L in enumerate(lens):
            for k in range(h):
                qs = slice(k * d, (k + 1) * d)
                ref[b][:, qs], l, vmax = H.attend(Q[b][:, qs], K[b][:, qs], V[b][:, qs], L, H.SCALES)
                bound[b][:, qs] = (H.FLIPS * 2.0 ** 4 * vmax / l)[:, None] + H.fp32_term(V, H.SCALES)
        print(f"{name} d {d} Nq {nq}: O worst err / bound = {H.compare(name, got, ref, bound):.3f}")
        if name == "zero_v":
            assert (got == 0).all()
        if name == "const":
            H.compare("const against the float64 mean", got, H.uniform_mean(Q, K, V, lens, h, hk, H.SCALES), H.fp32_term(V, H.SCALES))


@pytest.mark.parametrize("h,hk,nq", H.HEADS)
@FAMILY
@EACH_D
def test_family_decode(dev, d, name, h, hk, nq):
    worst = [0.0, 0.0]
    for kind in ("edge", "mid"):
        lens = H.lens_of(nq, kind)
        Q, K, V = H.family(name, d, h, hk, nq, lens)
        Qd, plain, paged = torch.from_numpy(Q).to(dev), full_cache(dev, K, V, d, h, hk), full_cache(dev, K, V, d, h, hk, page_rows=64)
        for chunk in H.CHUNKS:
            got, scratch = decode(*plain, Qd, lens, chunk)
            worst = np.maximum(worst, hold(f"{name} {kind} chunk {chunk}", got, scratch, H.decode(Q, K, V, lens, h, hk, H.SCALES, chunk, CAP), d, h, V))
            pgot, pscratch = decode(*paged, Qd, lens, chunk)
            assert_bits("paged against contiguous", pgot, got), H.same_bits("paged against contiguous: the scratch", pscratch, scratch)
            if name == "zero_v":
                assert (got == 0).all()
            if name == "const":
                H.compare("const against the float64 mean", got, H.uniform_mean(Q, K, V, lens, h, hk, H.SCALES), H.fp32_term(V, H.SCALES))
    print(f"{name} d {d} h {h}/{hk} Nq {nq}: worst err / bound O = {worst[0]:.3f}, partials = {worst[1]:.3f}")


@pytest.mark.parametrize("h,hk,nq", H.HEADS)
@FAMILY
@EACH_D
def test_family_decode_window(dev, d, name, h, hk, nq):
    worst = [0.0, 0.0]
    for kind in ("edge", "mid"):
        lens = H.lens_of(nq, kind)
        Q, K, V = H.family(name, d, h, hk, nq, lens)
        Qd, plain, paged = torch.from_numpy(Q).to(dev), full_cache(dev, K, V, d, h, hk), full_cache(dev, K, V, d, h, hk, page_rows=64)
        for chunk, window, sinks in ((c, w, s) for c in H.CHUNKS for w in H.WINDOWS for s in (None, H.ramp(h))):
            got, scratch = decode(*plain, Qd, lens, chunk, window, sinks)
            want = H.decode(Q, K, V, lens, h, hk, H.SCALES, chunk, CAP, window, sinks)
            worst = np.maximum(worst, hold(f"{name} {kind} chunk {chunk} window {window} sinks {sinks is not None}", got, scratch, want, d, h, V))
            pgot, pscratch = decode(*paged, Qd, lens, chunk, window, sinks)
            assert_bits("paged against contiguous", pgot, got), H.same_bits("paged against contiguous: the scratch", pscratch, scratch)
            if name == "zero_v":
                assert (got == 0).all()
            if name == "const" and sinks is None:
                H.compare("const against the float64 mean", got, H.uniform_mean(Q, K, V, lens, h, hk, H.SCALES, window), H.fp32_term(V, H.SCALES))
    print(f"{name} d {d} h {h}/{hk} Nq {nq}: worst err / bound O = {worst[0]:.3f}, partials = {worst[1]:.3f}")


@pytest.mark.parametrize("name", ["rise", "spike", "normal"])
@pytest.mark.parametrize("h,hk,nq", H.HEADS)
@EACH_D
def test_sinks_at_the_clamp_and_at_zero(dev, d, h, hk, nq, name):
    """Sinks 130 log2 units and more above every score (the exponent's clamp at 120): the term is 2^120, so O is
    the restatement's small but normal number -- within H.compare_sunk's bound, which shrinks with the keys' share of the row,
    and not the 0 of a term that overflowed.  Sinks of -1e4 (the term is 0): the null-sinks call's bits.  Both forms."""
    lens = H.lens_of(nq, "mid")
    Q, K, V = H.family(name, d, h, hk, nq, lens)
    Qd, cache = torch.from_numpy(Q).to(dev), full_cache(dev, K, V, d, h, hk)
    high, low = H.high_sinks(Q, K, V, lens, h, hk, CAP), np.full(h, -1e4, np.float32)
    for chunk, window in ((128, 33), (64, 100), (64, 1000)):
        assert (dwr.chunks(CAP, nq, window, chunk) == 1) == (chunk == 128)
        got, scratch = decode(*cache, Qd, lens, chunk, window, high)
        want = H.decode(Q, K, V, lens, h, hk, H.SCALES, chunk, CAP, window, high)
        _, wp = hold(f"{name} chunk {chunk} window {window}, high sinks", got, scratch, want, d, h, V)
        keys = H.decode(Q, K, V, lens, h, hk, H.SCALES, chunk, CAP, window)[2]  # the row sums without the sink term
        wo = H.compare_sunk(f"{name} chunk {chunk} window {window}, high sinks", got, (want[0], None, want[2], want[3]), keys, d, H.fp32_term(V, H.SCALES))
        print(f"{name} chunk {chunk} window {window}: high sinks, worst err / bound O = {wo:.3f}, partials = {wp:.3f}, max|O| = {float(np.abs(got).max()):.3e}")
        assert float(np.abs(got).max()) <= 2.0 ** -100 * float(np.abs(V).max())
        assert_bits("sinks of -1e4 against no sinks", decode(*cache, Qd, lens, chunk, window, low)[0], decode(*cache, Qd, lens, chunk, window)[0])


# ---- c. multi-stage chunks and large pages at B = 2, cap 768 -------------------------------------------------------------
BIG = pytest.mark.parametrize("h,hk,nq", H.BIG_HEADS)
DIST = pytest.mark.parametrize("name", ["normal", "rise"])
LENS = pytest.mark.parametrize("li", [0, 1, 2])


def nan_behind(cache, table, lens, d, hk, page_rows=None, first=None):
    """0x7f (the e4m3 NaN byte) in every cache byte of a row at or behind ceil32(lens[b]) (or before first[b]), and in the page no
    sequence has."""
    nb, cap = len(lens), H.BIG_CAP
    rows, slices = (cap, nb * hk) if page_rows is None else (page_rows, (nb * (cap // page_rows) + 1) * hk)
    keep = np.zeros((2, slices, rows, d), bool)
    T = None if page_rows is None else table_of(nb, cap // page_rows)
    for b, L in enumerate(lens):
        for r0 in range(first[b] if first else 0, -(-L // 32) * 32, 32):
            sl, at = (b, r0) if T is None else (int(T[b][r0 // page_rows]), r0 % page_rows)
            keep[:, sl * hk:(sl + 1) * hk, at:at + 32] = True
    assert cache.mem.numel() == keep.size
    cache.mem[torch.from_numpy(~keep.ravel()).to(cache.mem.device)] = 0x7F
    return cache, table


@LENS
@DIST
@BIG
@EACH_D
def test_multi_stage_decode(dev, d, h, hk, nq, name, li):
    """chunk_rows 192, 256, 320 and 768 (3, 4, 5 and 12 stages a chunk): O and the partials against the restatement; the paged call
    at 64, 128, 192 and 384-row pages, O and scratch bit for bit; NaN bytes behind the rows, a guard behind O and the scratch."""
    lens, cap = H.big_lens(nq)[li], H.BIG_CAP
    Q, K, V = H.family(name, d, h, hk, nq, lens, cap)
    Qd, plain = torch.from_numpy(Q).to(dev), nan_behind(*fill(*new_cache(dev, H.BIG_B, cap, d, h, hk, H.SCALES), K, V, lens), lens, d, hk)
    pools = [nan_behind(*fill(*new_cache(dev, H.BIG_B, cap, d, h, hk, H.SCALES, pr), K, V, lens), lens, d, hk, pr) for pr in H.BIG_PAGES]
    worst = [0.0, 0.0]
    for chunk in H.BIG_CHUNKS:
        got, scratch = decode(*plain, Qd, lens, chunk, guard=4096)
        worst = np.maximum(worst, hold(f"{name} lens {lens} chunk {chunk}", got, scratch, H.decode(Q, K, V, lens, h, hk, H.SCALES, chunk, cap), d, h, V))
        for pr, pool in zip(H.BIG_PAGES, pools):
            pgot, pscratch = decode(*pool, Qd, lens, chunk, guard=4096)
            assert_bits(f"chunk {chunk}, {pr}-row pages against contiguous", pgot, got), H.same_bits(f"chunk {chunk}, {pr}-row pages: the scratch", pscratch, scratch)
        for r in range(nq if nq > 1 else 0):  # the same tiles, the same mask, the same streams
            one, _ = decode(*plain, Qd[:, r:r + 1].contiguous(), [L - nq + 1 + r for L in lens], chunk)
            assert_bits(f"chunk {chunk}: row {r} against the one-row call", got[:, r:r + 1], one)
    print(f"{name} d {d} h {h}/{hk} Nq {nq} lens {lens}: worst err / bound O = {worst[0]:.3f}, partials = {worst[1]:.3f}")


@pytest.mark.parametrize("pr", H.BIG_PAGES)
@DIST
@EACH_D
def test_prefill_on_large_pages(dev, d, name, pr):
    """attend_paged at Nq = 40 on 64 ... 384-row pages against attend_tokens, bit for bit."""
    (h, hk), nq, lens, cap = (4, 2), 40, (449, 768), H.BIG_CAP
    Q, K, V = H.family(name, d, h, hk, nq, lens, cap)
    Qd = torch.from_numpy(Q).to(dev)
    want = prefill(*nan_behind(*fill(*new_cache(dev, H.BIG_B, cap, d, h, hk, H.SCALES), K, V, lens), lens, d, hk), Qd, lens)
    got = prefill(*nan_behind(*fill(*new_cache(dev, H.BIG_B, cap, d, h, hk, H.SCALES, pr), K, V, lens), lens, d, hk, pr), Qd, lens)
    assert_bits(f"{pr}-row pages against contiguous", got, want)


@LENS
@DIST
@BIG
@EACH_D
def test_multi_stage_decode_window(dev, d, h, hk, nq, name, li):
    """Window 128 at chunk_rows 256 (one launch, up to four stages from a t0 > 0, the scratch untouched) and at 64 (combine);
    window 500 at 192; window 1024 >= cap at 192: attend_decode's bits without sinks.  Contiguous and 128-row pages."""
    lens, cap = H.big_lens(nq)[li], H.BIG_CAP
    Q, K, V = H.family(name, d, h, hk, nq, lens, cap)
    Qd, plain = torch.from_numpy(Q).to(dev), nan_behind(*fill(*new_cache(dev, H.BIG_B, cap, d, h, hk, H.SCALES), K, V, lens), lens, d, hk)
    pool = nan_behind(*fill(*new_cache(dev, H.BIG_B, cap, d, h, hk, H.SCALES, 128), K, V, lens), lens, d, hk, 128)
    tight = nan_behind(*fill(*new_cache(dev, H.BIG_B, cap, d, h, hk, H.SCALES), K, V, lens), lens, d, hk, first=[32 * dwr.first_tile(L, nq, 128) for L in lens])
    worst = [0.0, 0.0]
    for window, chunk in H.BIG_WINDOWS:
        NC = dwr.chunks(cap, nq, window, chunk)
        assert (NC == 1) == ((window, chunk) == (128, 256))
        for sinks in (None, H.ramp(h)):
            got, scratch = decode(*plain, Qd, lens, chunk, window, sinks, guard=4096)
            assert NC > 1 or np.isnan(scratch).all(), "the one-launch form wrote into the scratch"
            want = H.decode(Q, K, V, lens, h, hk, H.SCALES, chunk, cap, window, sinks)
            worst = np.maximum(worst, hold(f"{name} lens {lens} window {window} chunk {chunk} sinks {sinks is not None}", got, scratch, want, d, h, V))
            pgot, pscratch = decode(*pool, Qd, lens, chunk, window, sinks, guard=4096)
            assert_bits(f"window {window} chunk {chunk}: 128-row pages against contiguous", pgot, got), H.same_bits("the scratch", pscratch, scratch)
            if window == 128:  # NaN bytes in the rows before 32 t0 too
                assert_bits(f"window 128 chunk {chunk}: NaN bytes outside the swept rows", decode(*tight, Qd, lens, chunk, window, sinks)[0], got)
            if window >= cap and sinks is None:
                assert_bits("window >= cap against attend_decode", got, decode(*plain, Qd, lens, chunk)[0])
    print(f"{name} d {d} h {h}/{hk} Nq {nq} lens {lens}: worst err / bound O = {worst[0]:.3f}, partials = {worst[1]:.3f}")
