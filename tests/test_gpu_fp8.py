"""GPU tests of the e4m3 K/V cache variant fa_tc_fp8 against its numpy restatement (tests/fp8_ref.py).

B = 3, cap 224 (its last two-tile stage is partial; the pool: 4 columns of 64-row pages under a permuted table).  O is held
to the restatement within FLIPS one-flip units u_r = 2^-4 * 2^8 * max|v| / l_r plus 2^-16 max|V| for fp32 (256 keys'
accumulation at 2^-24 each).  A P entry on an e4m3 rounding boundary moves one step, at most 2^-4 * 2^8 for p <= 2^8: one
unit.  FLIPS = 2, the int8 suites' constant: one such flip in a row and a second one as margin."""
import functools

import numpy as np
import pytest
import torch

from tests import fp8_ref
from tests import rect_ref as rr
from tests.gpu_support import GUARD, Guarded, assert_bits, assert_zeros, compiled_module, dev, i32  # noqa: F401

pytestmark = pytest.mark.gpu
FP8, B, CAP, FILL, FLIPS = "fa_tc_fp8", 3, 224, 0x5A, 2.0
UNIT, SCALES = (1.0, 1.0, 1.0), (0.3, 0.7, 1.9)  # no power of two: x / scale is an IEEE division or the bytes differ
GEOS = {"mh": (2, 2, False), "gqa2": (4, 2, False), "gqa1": (4, 1, False), "paged": (2, 2, True), "mh4": (4, 4, False)}  # h, h_kv, paged
SHAPES = [(1, (33, 95, 224)), (5, (33, 95, 224)), (32, (40, 100, 224)), (40, (40, 100, 224))]  # Nq, lengths
TABLE, PAGES = [[6, 2, 9, 4], [1, 11, 0, 7], [8, 3, 10, 5]], 13  # page 12 is in no sequence
EVERY = pytest.mark.parametrize("d,geo", [(d, g) for d in (64, 128) for g in ("mh", "gqa2", "gqa1", "paged")])
EACH_D = pytest.mark.parametrize("d", [64, 128])


@functools.lru_cache(maxsize=None)
def inputs(d, geo, nq, dist="normal"):
    """Q [B, nq, h d], K, V [B, CAP, h_kv d], the same K, V for every nq; "mh4": gqa2's K / V with every head repeated twice."""
    h, hk, _ = GEOS[geo]
    _, K, V = rr.inputs(1, CAP, (2 if geo == "mh4" else hk) * d, B, dist, 12)
    if geo == "mh4":
        K, V = (np.repeat(x.reshape(B, CAP, 2, d), 2, axis=2).reshape(B, CAP, 4 * d) for x in (K, V))
    return rr.inputs(nq, CAP, h * d, B, dist, 11)[0], K, V


@functools.lru_cache(maxsize=None)
def build(dev, d, geo, lens, scales, dist="normal", mod=None):
    """A cache holding lens[b] rows of sequence b, appended in pieces of 17, 1, 46 and 64 rows over a sentinel."""
    from quantizedmha_amd import torch_ext
    mod, (h, hk, paged), (_, K, V) = mod or torch_ext, GEOS[geo], inputs(d, geo, 1, dist)
    if paged:
        cache, table = mod.PagedKVCache(B, PAGES, 64, 4, h * d, h, hk, FP8, str(dev)), i32(dev, TABLE)
    else:
        cache, table = mod.GroupedKVCache(B, CAP, h * d, h, hk, FP8, str(dev)) if hk < h else mod.KVCache(B, CAP, h * d, h, FP8, str(dev)), None
    cache.mem.fill_(FILL), cache.set_scales(*scales), cache.enable_tokens()
    assert cache.tail is None
    for b, L in enumerate(lens):
        p = 0
        for n in (17, 1, 46) + (64,) * 4:
            n = min(n, L - p)
            if n > 0:
                Kn, Vn = (torch.from_numpy(np.ascontiguousarray(np.broadcast_to(x[b, p:p + n], (B, n, hk * d)))).to(dev) for x in (K, V))
                pos = i32(dev, [p if i == b else -1 for i in range(B)])
                cache.append_paged(Kn, Vn, pos, table) if paged else cache.append_tokens(Kn, Vn, pos)
                p += n
    return cache, table


def expected_mem(nbytes, d, geo, lens, scales):
    """cache.mem of build(): the restatement's bytes in the groups below ceil32(L), the sentinel everywhere else."""
    (_, hk, paged), (_, K, V) = GEOS[geo], inputs(d, geo, 1)
    rows, slices = (64, PAGES * hk) if paged else (CAP, B * hk)
    exp, vo = np.full(nbytes, FILL, np.uint8), slices * rows * d
    assert nbytes == 2 * vo
    for b, L in enumerate(lens):
        for kh in range(hk):
            k8, vt, _ = fp8_ref.cache_arrays(K[b][:, kh * d:(kh + 1) * d], V[b][:, kh * d:(kh + 1) * d], L, scales[1], scales[2])
            for g in range(len(k8) // 32):
                page, gp = (TABLE[b][g // 2], g % 2) if paged else (b, g)
                at = ((page * hk + kh) * rows + 32 * gp) * d
                exp[at:at + 32 * d], exp[vo + at:vo + at + 32 * d] = k8[32 * g:32 * g + 32].ravel(), vt[32 * g * d:32 * (g + 1) * d]
    return exp


def attend(cache, table, Q, lens):
    g = Guarded(Q)
    (cache.attend_tokens if table is None else cache.attend_paged)(Q, i32(Q.device, lens), *([] if table is None else [table]), out=g.buf[:g.n])
    return g.result()


@functools.lru_cache(maxsize=None)
def reference(d, geo, nq, lens, dist, causal=True):
    """The restatement's O in float64, the bound FLIPS u_r + fp32 per element, and float64 attention on the raw inputs."""
    (h, hk, _), (Q, K, V) = GEOS[geo], inputs(d, geo, nq, dist)
    ref, bound, exact = (np.zeros(Q.shape) for _ in range(3))
    for b, L in enumerate(lens):
        for k in range(h):
            kh, qs = k // (h // hk), slice(k * d, (k + 1) * d)
            Kb, Vb = K[b][:L, kh * d:(kh + 1) * d], V[b][:L, kh * d:(kh + 1) * d]
            k8, _, v8 = fp8_ref.cache_arrays(Kb, Vb, L, SCALES[1], SCALES[2])
            ref[b][:, qs], l, vmax = fp8_ref.attend(*(fp8_ref.decode(a) for a in (fp8_ref.encode(Q[b][:, qs], SCALES[0]), k8, v8)), L, SCALES, causal=causal)
            bound[b][:, qs] = (FLIPS * 2.0 ** 4 * vmax / l)[:, None] + 2.0 ** -16 * float(np.abs(V).max())
            s = (Q[b][:, qs].astype(np.float64) @ Kb.T.astype(np.float64)) / np.sqrt(d)
            if causal:
                s[np.arange(L)[None, :] > (np.arange(nq) + L - nq)[:, None]] = -np.inf
            p = np.exp(s - s.max(axis=1, keepdims=True))
            exact[b][:, qs] = (p @ Vb.astype(np.float64)) / p.sum(axis=1, keepdims=True)
    return ref, bound, exact


@pytest.mark.parametrize("scales", [UNIT, SCALES])
@pytest.mark.parametrize("lens", [SHAPES[0][1], SHAPES[2][1]])
@EVERY
def test_cache_bytes(dev, d, geo, lens, scales):
    got = build(dev, d, geo, lens, scales)[0].mem.cpu().numpy()
    want = expected_mem(got.size, d, geo, lens, scales)
    assert np.array_equal(got, want), (int((got != want).sum()), np.flatnonzero(got != want)[:8])


@pytest.mark.parametrize("dist", ["normal", "uniform"])
@pytest.mark.parametrize("nq,lens", SHAPES)
@EVERY
def test_o_against_restatement_and_float64(dev, d, geo, nq, lens, dist):
    got = attend(*build(dev, d, geo, lens, SCALES, dist), torch.from_numpy(inputs(d, geo, nq, dist)[0]).to(dev), lens).astype(np.float64)
    ref, bound, exact = reference(d, geo, nq, lens, dist)
    assert np.isfinite(got).all() and (np.abs(got - ref) <= bound).all(), float((np.abs(got - ref) / bound).max())
    sees = np.stack([np.arange(nq) + L - nq + 1 >= 33 for L in lens])  # rows with at least 33 keys
    far, own = np.abs(got - exact)[sees].max(), np.abs(ref - exact)[sees].max()
    assert far <= 1.25 * own, (far, own)  # the restatement's own distance from float64, never the kernel's


@EVERY
def test_isolation(dev, d, geo):
    """NaN bytes (0x7f) behind ceil32(L) and in unused pages leave every bit; an invalid length or table entry gives zeros."""
    nq, lens = 5, SHAPES[2][1]
    cache, table = build.__wrapped__(dev, d, geo, lens, SCALES)
    Q = torch.from_numpy(inputs(d, geo, nq)[0]).to(dev)
    want = attend(cache, table, Q, lens)
    cache.mem[torch.from_numpy(expected_mem(cache.mem.numel(), d, geo, lens, SCALES) == FILL).to(dev)] = 0x7F
    assert_bits("NaN bytes behind the rows", attend(cache, table, Q, lens), want)
    got = attend(cache, table, Q, [0, 100, 300])
    assert_bits("between two invalid lengths", got[1], want[1]), assert_zeros("lens 0", got[0]), assert_zeros("lens 300", got[2])
    if table is not None:
        got = attend(cache, i32(dev, [TABLE[0], [1, PAGES, 0, 7], TABLE[2]]), Q, lens)
        assert_zeros("a used entry outside the pool", got[1]), assert_bits("beside it", got[[0, 2]], want[[0, 2]])


@pytest.mark.parametrize("nq,lens", SHAPES)
@EACH_D
def test_paged_and_grouped_bits(dev, d, nq, lens):
    o = lambda geo: attend(*build(dev, d, geo, lens, SCALES), torch.from_numpy(inputs(d, geo, nq)[0]).to(dev), lens)  # noqa: E731
    assert_bits("paged against contiguous", o("paged"), o("mh"))
    assert_bits("grouped against the multi-head cache on repeated K / V", o("gqa2"), o("mh4"))


@pytest.mark.parametrize("geo", ["mh", "gqa2"])
@EACH_D
def test_whole_group_entry_points(dev, d, geo):
    """append_at + attend_varlen at multiples of 32 give attend_tokens' bits; append + the unmasked attend at len == cap."""
    from quantizedmha_amd import torch_ext
    (h, hk, _), (Q, K, V) = GEOS[geo], (torch.from_numpy(x).to(dev) for x in inputs(d, geo, 32))
    at, full = (torch_ext.GroupedKVCache(B, cap, h * d, h, hk, FP8, str(dev)) for cap in (CAP, 96))
    at.set_scales(*SCALES), full.set_scales(*SCALES)
    at.append_at(K[:, :96].contiguous(), V[:, :96].contiguous(), i32(dev, [0, 0, 0]))
    at.append_at(K[:, :32].contiguous(), V[:, :32].contiguous(), i32(dev, [36, -32, 224]))  # invalid rows: nothing is written
    full.append(K[:, :64].contiguous(), V[:, :64].contiguous()), full.append(K[:, 64:96].contiguous(), V[:, 64:96].contiguous())
    g = Guarded(Q)
    at.attend_varlen(Q, i32(dev, [64, 96, 40]), causal=True, out=g.buf[:g.n])
    got, want = g.result(), attend(*build(dev, d, geo, (96, 96, 96), SCALES), Q, (64, 96, 96))
    assert_bits("attend_varlen", got[:2], want[:2]), assert_zeros("lens 40", got[2])
    g = Guarded(Q)
    full.attend(Q, causal=False, out=g.buf[:g.n])
    ref, bound, _ = reference(d, geo, 32, (96, 96, 96), "normal", causal=False)
    assert full.len == 96 and (np.abs(g.result() - ref) <= bound).all()


def test_decode_step_under_graph_replay(dev):
    """One decode step captured once on a side stream, replayed across a group boundary (rows 30 .. 34, 62 .. 66; an empty slot)."""
    d, geo, start = 64, "mh", [30, 62, 0]
    Q, K, V = (torch.from_numpy(x).to(dev) for x in inputs(d, geo, 40))
    graphed, eager = (build.__wrapped__(dev, d, geo, start, SCALES)[0] for _ in range(2))
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        qs, ks, vs = (torch.zeros((B, 1, 2 * d), dtype=torch.float32, device=dev) for _ in range(3))
        buf = torch.full((qs.numel() + 32 * 2 * d,), GUARD, dtype=torch.float32, device=dev)
        pos, lens, inc = i32(dev, [-1] * B), i32(dev, [0] * B), i32(dev, [1, 1, 0])
        step = lambda: (graphed.append_tokens(ks, vs, pos), graphed.attend_tokens(qs, lens, out=buf[:qs.numel()]))  # noqa: E731
        step()  # once before the capture: every sequence invalid
        pos.copy_(i32(dev, start[:2] + [-1])), lens.copy_(i32(dev, [L + 1 for L in start[:2]] + [0]))
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            step()
        for k in range(5):
            qs.copy_(Q[:, k:k + 1])
            for x, X in ((ks, K), (vs, V)):
                x.copy_(torch.stack([X[b, L + k:L + k + 1] for b, L in enumerate(start)]))
            graph.replay()
            got = buf.clone()
            eager.append_tokens(ks, vs, pos)
            want = attend(eager, None, qs, lens.tolist())
            assert bool((got[qs.numel():] == GUARD).all()), "O written past its last row"
            assert_bits(f"replay {k}", got[:qs.numel()].view(qs.shape).cpu().numpy(), want), assert_zeros("the empty slot", want[2])
            pos.add_(inc), lens.add_(inc)
        side.synchronize()
    torch.cuda.current_stream(dev).wait_stream(side)
    assert_bits("the caches", graphed.mem.cpu().numpy(), eager.mem.cpu().numpy())


def test_compiled_module(dev):
    d, geo, (nq, lens) = 64, "gqa2", SHAPES[1]
    Q = torch.from_numpy(inputs(d, geo, nq)[0]).to(dev)
    cache, _ = build.__wrapped__(dev, d, geo, lens, SCALES, mod=compiled_module())
    got = cache.attend_tokens(Q, i32(dev, lens))
    torch.cuda.synchronize()
    assert_bits("compiled against ctypes", got.cpu().numpy(), attend(*build(dev, d, geo, lens, SCALES), Q, lens))
    with pytest.raises(RuntimeError, match="sliding window is not built for a fa_tc_fp8 cache"):
        cache.attend_tokens_window(Q, i32(dev, lens), 32)
