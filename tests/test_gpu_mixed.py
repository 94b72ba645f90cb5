"""GPU tests of the fp8 cache's mixed-step calls: B = 5 sequences in one packed step over a cache of 224 rows
(contiguous, or 64-row pages under a permuted table) -- 150 rows of chunked prefill (two unit blocks at G = 1), one decode row,
an empty slot whose lens / pos hold garbage, 40 rows, and k rows with G k = 32 (the widest decode kind) or G k + G > 32 (the
prefill kind just above it).  Every sequence's rows of O are held, bit for bit, to the shipped call of its kind on a batch in
which only that sequence is valid, and to float64 band attention with sinks on the decoded e4m3 operands within the sum of
the project's two bounds: (2^-4 + L 2^-18) max|v| (tests/test_fp8_cpu.py: restatement to float64) and FLIPS one-flip units
2^-4 2^8 max|v| / l plus 2^-16 max|V| (kernel to restatement), l the float64 row sum with the sink in it."""
import functools

import numpy as np
import pytest
import torch

from tests import fp8_ref
from tests import rect_ref as rr
from tests.gpu_support import GUARD, Guarded, assert_bits, assert_zeros, compiled_module, dev, i32  # noqa: F401
from tests.test_gpu_decode import CAP, FLIPS, FP8, SCALES
from tests.test_gpu_decode_window import ramp

pytestmark = pytest.mark.gpu
B, PAD, LENS = 5, 3, (200, 65, -7, 224, 193)  # PAD: rows of the packed operands behind the last range
TABLE, PAGES = [[6, 2, 9, 4], [1, 11, 0, 7], [8, 3, 10, 5], [12, 20, 14, 15], [19, 18, 17, 16]], 22  # pages 13, 21: in no sequence
WINDOWS, CHUNKS = (1, 33, 100, 1000), (64, 128)
CASES = pytest.mark.parametrize("d,paged,h,hk", [(d, p, h, hk) for d in (64, 128) for p in (False, True) for h, hk in ((2, 2), (4, 1), (8, 2))])


def counts(G, over):
    return [150, 1, 0, 40, 32 // G + over]


@functools.lru_cache(maxsize=None)
def inputs(d, h, hk, total):
    """Q [total, h d]; K, V [B, CAP, hk d]"""
    _, K, V = rr.inputs(1, CAP, hk * d, B, "normal", 12)
    return rr.inputs(total, CAP, h * d, 1, "normal", 11)[0][0], K, V


def first_row(L, nq, window, G):
    """The first row a sequence's shipped call stages: the decode kind's, or the prefill kind's first unit block's."""
    return max(0, (L - nq - window + 1) if G * nq <= 32 else ((L - nq) // 32 * 32 - window + 1)) // 64 * 64


def make(dev, d, h, hk, K, V, n, paged, mixed, fill=0, first=(0,) * B, mod=None):
    """A cache over `fill` bytes holding rows [first[b], LENS[b]): the history by the shipped appends, the step's last n[b] rows
    by append_mixed (mixed) or by the shipped append at n = n[b] with every other sequence switched off; (cache, table)."""
    from quantizedmha_amd import torch_ext
    mod = mod or torch_ext
    cache = mod.PagedKVCache(B, PAGES, 64, 4, h * d, h, hk, FP8, str(dev)) if paged else mod.GroupedKVCache(B, CAP, h * d, h, hk, FP8, str(dev))
    table = i32(dev, TABLE) if paged else None
    cache.mem.fill_(fill), cache.set_scales(*SCALES), cache.enable_tokens()

    def shipped(b, lo, hi):
        if hi > lo:
            Kn, Vn = (torch.from_numpy(np.ascontiguousarray(np.broadcast_to(x[b, lo:hi], (B, hi - lo, hk * d)))).to(dev) for x in (K, V))
            pos = i32(dev, [lo if i == b else -1 for i in range(B)])
            cache.append_paged(Kn, Vn, pos, table) if paged else cache.append_tokens(Kn, Vn, pos)

    live = [b for b in range(B) if n[b]]
    for b in live:
        shipped(b, first[b], LENS[b] - n[b])
    if mixed:
        Kp, Vp = (torch.from_numpy(np.concatenate([x[b, LENS[b] - n[b]:LENS[b]] for b in live] + [np.full((PAD, hk * d), np.nan, np.float32)])).to(dev)
                  for x in (K, V))
        cu, pos = i32(dev, np.concatenate([[0], np.cumsum(n)])), i32(dev, [LENS[b] - n[b] for b in range(B)])  # the empty slot: pos = -7
        cache.append_paged_mixed(Kp, Vp, cu, pos, table) if paged else cache.append_mixed(Kp, Vp, cu, pos)
    else:
        for b in live:
            shipped(b, LENS[b] - n[b], LENS[b])
    return cache, table


def attend(cache, table, Q, cu, lens, window, sinks=None):
    """attend_mixed through the guard behind O, over a NaN scratch with a guard of its own; O (numpy)."""
    g, s = Guarded(Q), None if sinks is None else torch.from_numpy(sinks).to(Q.device)
    size = cache.mixed_scratch.numel()
    cache.mixed_scratch = torch.full((size + 4096,), 0xFF, dtype=torch.uint8, device=Q.device)
    if table is None:
        cache.attend_mixed(Q, cu, i32(Q.device, lens), window, s, out=g.out)
    else:
        cache.attend_paged_mixed(Q, cu, i32(Q.device, lens), table, window, s, out=g.out)
    got = g.result()
    assert bool((cache.mixed_scratch[size:] == 0xFF).all()), "the scratch written past its last byte"
    cache.mixed_scratch = cache.mixed_scratch[:size]
    return got


def shipped_attend(cache, table, Qb, b, L, window, sinks, chunk, G):
    """Sequence b's rows by the shipped call of its kind: a batch at Nq = nq_b in which every other sequence is invalid."""
    nq, dev_ = Qb.shape[0], Qb.device
    Q = torch.zeros((B, nq, Qb.shape[1]), dtype=torch.float32, device=dev_)
    Q[b] = Qb
    g, s, lens, args = Guarded(Q), None if sinks is None else torch.from_numpy(sinks).to(dev_), i32(dev_, [L if i == b else 0 for i in range(B)]), [] if table is None else [table]
    if G * nq <= 32:
        cache.enable_decode_window(chunk, 1000, nq)
        (cache.attend_decode_window if table is None else cache.attend_paged_decode_window)(Q, lens, *args, window, s, out=g.buf[:g.n])
    else:
        (cache.attend_prefill_window if table is None else cache.attend_paged_prefill_window)(Q, lens, *args, window, s, out=g.buf[:g.n])
    return g.result()[b]


def exact(Q, K, V, L, h, hk, window, sinks):
    """float64 band attention with sinks of one sequence on the decoded e4m3 operands: O [nq, h d] and the bound's terms."""
    nq, d, G = Q.shape[0], Q.shape[1] // h, h // hk
    O, bound = np.zeros(Q.shape), np.zeros(Q.shape)
    e, j = (np.arange(nq) + L - nq)[:, None], np.arange(L)[None, :]
    lo = first_row(L, nq, window, G)
    for k in range(h):
        kh, qs = k // G, slice(k * d, (k + 1) * d)
        k8, _, v8 = fp8_ref.cache_arrays(K[:L, kh * d:(kh + 1) * d], V[:L, kh * d:(kh + 1) * d], L, SCALES[1], SCALES[2])
        q, kk, v = (fp8_ref.decode(a).astype(np.float64) for a in (fp8_ref.encode(Q[:, qs], SCALES[0]), k8[:L], v8[:L]))
        s = (q @ kk.T) * SCALES[0] * SCALES[1] / np.sqrt(d)
        s[(j > e) | (j <= e - window)] = -np.inf
        mx = s.max(axis=1, keepdims=True)
        p = np.exp(s - mx)
        den = p.sum(axis=1, keepdims=True) + (0.0 if sinks is None else np.exp(sinks[k] - mx))
        O[:, qs] = SCALES[2] * (p @ v) / den
        vmax = np.abs(v[lo:]).max() * SCALES[2]
        bound[:, qs] = (2.0 ** -4 + L * 2.0 ** -18) * vmax + FLIPS * 2.0 ** 4 * vmax / (256.0 * den) + 2.0 ** -16 * float(np.abs(V).max())
    return O, bound


@pytest.mark.parametrize("over", [0, 1])
@CASES
def test_bits_and_float64(dev, d, paged, h, hk, over):
    G = h // hk
    n = counts(G, over)
    cu = np.concatenate([[0], np.cumsum(n)])
    Q, K, V = inputs(d, h, hk, int(cu[-1]) + PAD)
    (cache, table), (ref, _) = make(dev, d, h, hk, K, V, n, paged, True), make(dev, d, h, hk, K, V, n, paged, False)
    torch.cuda.synchronize()
    assert torch.equal(cache.mem, ref.mem), "append_mixed: the cache bytes are not the shipped appends'"
    cap = cache.cap  # the pool's logical capacity is 4 pages of 64 rows
    bad = i32(dev, [-1, cap, 0, cap - 39, cap - n[4] + 1])  # below 0; at cap; the empty slot; 40 and k rows one past the end
    Kp = torch.from_numpy(np.ones((int(cu[-1]) + PAD, hk * d), np.float32)).to(dev)
    cache.append_paged_mixed(Kp, Kp, i32(dev, cu), bad, table) if paged else cache.append_mixed(Kp, Kp, i32(dev, cu), bad)
    torch.cuda.synchronize()
    assert torch.equal(cache.mem, ref.mem), "append_mixed: an invalid pos wrote something"
    Qd, worst = torch.from_numpy(Q).to(dev), 0.0
    for chunk in CHUNKS:
        cache.enable_mixed(chunk, 1000)
        for window, sunk in ((w, s) for w in WINDOWS for s in (False, True)):
            sinks = ramp(h) if sunk else None
            got = attend(cache, table, Qd, i32(dev, cu), LENS, window, sinks)
            assert (got[cu[-1]:] == GUARD).all(), "rows outside every range were written"
            for b in (b for b in range(B) if n[b]):
                rows = slice(cu[b], cu[b + 1])
                assert_bits(f"chunk {chunk} window {window} sinks {sunk}: sequence {b} against the shipped call of its kind", got[rows],
                            shipped_attend(ref, table, Qd[rows], b, LENS[b], window, sinks, chunk, G))
                if chunk == CHUNKS[0]:
                    want, bound = exact(Q[rows], K[b], V[b], LENS[b], h, hk, window, sinks)
                    err = np.abs(got[rows] - want)
                    worst = max(worst, float((err / bound).max()))
                    assert (err <= bound).all(), (window, sunk, b, float((err / bound).max()))
    print(f"d {d} paged {paged} h {h} hk {hk} over {over}: worst |O - float64| / bound = {worst:.3f}")


@pytest.mark.parametrize("d,paged", [(64, False), (64, True), (128, True)])
def test_isolation(dev, d, paged):
    """NaN bytes wherever no staged row lies and -1 in the table's columns behind every band reach nothing; an invalid length,
    a range outside [0, total] and a table entry outside the pool touch their own sequence only."""
    (h, hk), window, chunk, sinks = (4, 1), 33, 64, ramp(4)
    n = counts(4, 0)
    cu = np.concatenate([[0], np.cumsum(n)])
    Q, K, V = inputs(d, h, hk, int(cu[-1]) + PAD)
    Qd, cud = torch.from_numpy(Q).to(dev), i32(dev, cu)
    full, table = make(dev, d, h, hk, K, V, n, paged, True)
    full.enable_mixed(chunk, window)
    want = attend(full, table, Qd, cud, LENS, window, sinks)
    first = tuple(first_row(L, nq, window, 4) if nq else 0 for L, nq in zip(LENS, n))
    assert first == (0, 0, 0, 128, 128)
    cache, _ = make(dev, d, h, hk, K, V, n, paged, True, fill=0x7F, first=first)  # e4m3 NaN bytes
    cache.enable_mixed(chunk, window)
    if paged:
        table = i32(dev, [[-1 if 64 * (c + 1) <= f else e for c, e in enumerate(row)] for row, f in zip(TABLE, first)])
    assert_bits("NaN bytes outside the staged rows, -1 behind the bands", attend(cache, table, Qd, cud, LENS, window, sinks), want)

    def others(label, got, zeroed, skipped=()):
        for b in (b for b in range(B) if n[b]):
            rows = slice(cu[b], cu[b + 1])
            if b in skipped:
                assert (got[rows] == GUARD).all(), (label, b, "written")
            elif b in zeroed:
                assert_zeros(f"{label}: sequence {b}", got[rows])
            else:
                assert_bits(f"{label}: sequence {b}", got[rows], want[rows])
        assert (got[cu[-1]:] == GUARD).all(), (label, "rows outside every range were written")

    others("lens below nq_b and above cap", attend(cache, table, Qd, cud, (149, 65, -7, 300, 7), window, sinks), zeroed=(0, 3, 4))
    out = cu.copy()
    out[-1] = cu[-1] + PAD + 1  # one row past total
    others("a range outside [0, total]", attend(cache, table, Qd, i32(dev, out), LENS, window, sinks), zeroed=(), skipped=(4,))
    if paged:
        bad = table.clone()
        bad[0, 1], bad[4, 3] = PAGES, -1  # rows 64 .. 127 of the prefill-kind sequence 0; rows 192 .. of the decode-kind sequence 4
        others("entries outside the pool among the read columns", attend(cache, bad, Qd, cud, LENS, window, sinks), zeroed=(0, 4))


@pytest.mark.parametrize("d,paged", [(64, False), (128, True)])
def test_graph_replay_follows_the_mix(dev, d, paged):
    """One step captured on one stream, replayed after cu is rewritten in device memory so that sequence 3 goes from the
    prefill kind (33 rows) to the decode kind (32) and back, against the eager call."""
    (h, hk), window, chunk = (2, 2), 100, 64
    mixes = [[40, 1, 0, 33, 1], [40, 1, 0, 32, 2], [8, 30, 5, 32, 0]]
    Q, K, V = inputs(d, h, hk, 75 + PAD)
    cache, table = make(dev, d, h, hk, K, V, [1, 1, 0, 1, 1], paged, False)  # rows [0, LENS[b]); sequence 2 stays zero bytes
    cache.enable_mixed(chunk, window)
    args, Qd, sinks = [] if table is None else [table], torch.from_numpy(Q).to(dev), torch.from_numpy(ramp(h)).to(dev)
    call = cache.attend_paged_mixed if paged else cache.attend_mixed
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        buf = torch.full((Qd.numel() + 32 * h * d,), GUARD, dtype=torch.float32, device=dev)
        out = buf[:Qd.numel()].view(Qd.shape)
        lens, cu = i32(dev, [200, 65, 70, 224, 193]), i32(dev, np.concatenate([[0], np.cumsum(mixes[0])]))
        call(Qd, cu, lens, *args, window, sinks, out=out)  # once before the capture
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            call(Qd, cu, lens, *args, window, sinks, out=out)
        for k, mix in enumerate(mixes + mixes[:1]):
            cu.copy_(i32(dev, np.concatenate([[0], np.cumsum(mix)])))
            buf.fill_(GUARD)
            graph.replay()
            got, want = buf.clone(), torch.full_like(Qd, GUARD)
            call(Qd, cu, lens, *args, window, sinks, out=want)
            assert bool((got[Qd.numel():] == GUARD).all()), "O written past its last row"
            assert_bits(f"replay {k}", got[:Qd.numel()].view(Qd.shape).cpu().numpy(), want.cpu().numpy())
            assert bool((want[:sum(mix)] != GUARD).all()) and bool((want[sum(mix):] == GUARD).all())
        side.synchronize()
    torch.cuda.current_stream(dev).wait_stream(side)


def test_compiled_module(dev):
    d, (h, hk), window, chunk = 64, (8, 2), 100, 64
    n = counts(4, 1)
    cu = np.concatenate([[0], np.cumsum(n)])
    Q, K, V = inputs(d, h, hk, int(cu[-1]) + PAD)
    Qd, sinks = torch.from_numpy(Q).to(dev), torch.from_numpy(ramp(h)).to(dev)
    for paged in (False, True):
        (cache, table), (ref, _) = make(dev, d, h, hk, K, V, n, paged, True, mod=compiled_module()), make(dev, d, h, hk, K, V, n, paged, True)
        cache.enable_mixed(chunk, window), ref.enable_mixed(chunk, window)
        args = [i32(dev, cu), i32(dev, LENS)] + ([table] if paged else [])
        got = (cache.attend_paged_mixed if paged else cache.attend_mixed)(Qd, *args, window, sinks)
        torch.cuda.synchronize()
        assert torch.equal(cache.mem, ref.mem), "compiled append against ctypes"
        assert_bits("compiled against ctypes", got.cpu().numpy()[:cu[-1]], attend(ref, table, Qd, args[0], LENS, window, ramp(h))[:cu[-1]])
    with pytest.raises(RuntimeError, match="fa_tc_fp8 cache"):
        compiled_module().GroupedKVCache(B, CAP, h * d, h, hk, "fa_tc_v1a", str(dev)).enable_mixed(chunk, window)
