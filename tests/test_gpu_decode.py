"""GPU tests of the fp8 cache's decode call against its numpy restatement (tests/decode_ref.py).

B = 3, cap 224 (the last two-tile stage and the last chunk are partial; the pool: 4 columns of 64-row pages under a permuted
table).  O and every partial the combine reads are held to the restatement within FLIPS one-flip units u = 2^-4 * 2^8 *
max|v| / l plus 2^-16 max|V| for fp32 -- the bound and constant of tests/test_gpu_fp8.py, l the restatement's
Ltot (O) or the partial's own l."""
import functools

import numpy as np
import pytest
import torch

from tests import decode_ref
from tests import rect_ref as rr
from tests.gpu_support import GUARD, Guarded, assert_bits, assert_zeros, compiled_module, dev, i32  # noqa: F401

pytestmark = pytest.mark.gpu
FP8, B, CAP, FLIPS, SCALES = "fa_tc_fp8", 3, 224, 2.0, (0.3, 0.7, 1.9)
TABLE, PAGES = [[6, 2, 9, 4], [1, 11, 0, 7], [8, 3, 10, 5]], 13  # page 12 is in no sequence
HEADS = [(2, 2, 1), (4, 1, 4), (4, 1, 5), (8, 2, 8)]  # h, h_kv, Nq: W = 1, 16, 20, 32 columns
EACH = pytest.mark.parametrize("d,chunk", [(64, 64), (64, 128), (128, 64), (128, 128)])
HNQ = pytest.mark.parametrize("h,hk,nq", HEADS)


def lens_of(nq, kind):
    return (nq, 65, 224) if kind == "edge" else (33, 95, 193)


@functools.lru_cache(maxsize=None)
def inputs(d, h, hk, nq, repeat=1):
    """Q [B, nq, h d]; K, V [B, CAP, hk d], with repeat > 1 every K/V head `repeat` times (a multi-head twin of a grouped cache)."""
    _, K, V = rr.inputs(1, CAP, hk * d, B, "normal", 12)
    if repeat > 1:
        K, V = (np.repeat(x.reshape(B, CAP, hk, d), repeat, axis=2).reshape(B, CAP, hk * repeat * d) for x in (K, V))
    return rr.inputs(nq, CAP, h * d, B, "normal", 11)[0], K, V


def make(dev, d, h, hk, K, V, lens, chunk, nq, paged=False, fill=0, mod=None):
    """A cache holding lens[b] rows of sequence b over `fill` bytes, with the decode scratch for nq rows; (cache, table)."""
    from quantizedmha_amd import torch_ext
    mod = mod or torch_ext
    cache = mod.PagedKVCache(B, PAGES, 64, 4, h * d, h, hk, FP8, str(dev)) if paged else mod.GroupedKVCache(B, CAP, h * d, h, hk, FP8, str(dev))
    table = i32(dev, TABLE) if paged else None
    cache.mem.fill_(fill), cache.set_scales(*SCALES), cache.enable_tokens(), cache.enable_decode(chunk, nq)
    for b, L in enumerate(lens):
        if L == 0:
            continue
        Kn, Vn = (torch.from_numpy(np.ascontiguousarray(np.broadcast_to(x[b, :L], (B, L, hk * d)))).to(dev) for x in (K, V))
        pos = i32(dev, [0 if i == b else -1 for i in range(B)])
        cache.append_paged(Kn, Vn, pos, table) if paged else cache.append_tokens(Kn, Vn, pos)
    return cache, table


def attend(cache, table, Q, lens):
    """O (numpy, through the guard) and the scratch as float32 (numpy)."""
    g = Guarded(Q)
    if table is None:
        cache.attend_decode(Q, i32(Q.device, lens), out=g.buf[:g.n])
    else:
        cache.attend_paged_decode(Q, i32(Q.device, lens), table, out=g.buf[:g.n])
    return g.result(), cache.decode_scratch.cpu().numpy().view(np.float32)


@functools.lru_cache(maxsize=None)
def reference(d, h, hk, nq, lens, chunk):
    Q, K, V = inputs(d, h, hk, nq)
    O, part, Ltot, vmax = decode_ref.decode(Q, K, V, lens, h, hk, SCALES, chunk, CAP)
    unit = FLIPS * 2.0 ** 4 * vmax, 2.0 ** -16 * float(np.abs(V).max())
    return O, part, Ltot, unit, decode_ref.exact(Q, K, V, lens, h, hk)


@pytest.mark.parametrize("kind", ["edge", "mid"])
@HNQ
@EACH
def test_against_restatement_and_float64(dev, d, chunk, h, hk, nq, kind):
    lens, (Q, K, V) = lens_of(nq, kind), inputs(d, h, hk, nq)
    cache, _ = make(dev, d, h, hk, K, V, lens, chunk, nq)
    cache.decode_scratch.fill_(0xFF)  # NaN: what the call leaves alone stays NaN
    got, scratch = attend(cache, None, torch.from_numpy(Q).to(dev), lens)
    ref, (Oc, pm, pl), Ltot, (unit, fp32), exact = reference(d, h, hk, nq, lens, chunk)
    per_head = lambda x: np.repeat(x, d, axis=-1)  # noqa: E731 -- [.., h] -> [.., h d]
    bound = per_head(unit[:, None, :] / Ltot) + fp32
    err = np.abs(got.astype(np.float64) - ref)
    print(f"O: worst err / bound = {float((err / bound).max()):.3f}")
    assert np.isfinite(got).all() and (err <= bound).all(), float((err / bound).max())
    gOc, gm, gl = decode_ref.views(scratch, B, -(-CAP // chunk), nq, h, d)
    assert np.array_equal(np.isnan(gl), np.isnan(pl)) and np.array_equal(np.isnan(gOc), np.isnan(Oc)) and np.array_equal(np.isnan(gm), np.isnan(pm))
    w = ~np.isnan(pl)
    perr, pbound = np.abs(gOc - Oc)[per_head(w)], (per_head(unit[:, None, None, :] / np.where(w, pl, 1.0)) + fp32)[per_head(w)]
    print(f"partials: worst err / bound = {float((perr / pbound).max()):.3f}")
    assert (perr <= pbound).all(), float((perr / pbound).max())
    sees = np.stack([np.arange(nq) + L - nq + 1 >= 33 for L in lens])  # rows with at least 33 keys
    if sees.any():
        far, own = np.abs(got - exact)[sees].max(), np.abs(ref - exact)[sees].max()
        assert far <= 1.25 * own, (far, own)  # the restatement's own distance from float64, never the kernel's


@HNQ
@EACH
def test_bit_identities(dev, d, chunk, h, hk, nq):
    lens, (Q, K, V) = lens_of(nq, "edge"), inputs(d, h, hk, nq)
    Qd = torch.from_numpy(Q).to(dev)
    want, scratch = attend(*make(dev, d, h, hk, K, V, lens, chunk, nq), Qd, lens)
    got, pscratch = attend(*make(dev, d, h, hk, K, V, lens, chunk, nq, paged=True), Qd, lens)
    assert_bits("paged against contiguous", got, want)
    assert np.array_equal(pscratch.view(np.uint32), scratch.view(np.uint32)), "paged against contiguous: the scratch"
    if hk < h:
        _, Kr, Vr = inputs(d, h, hk, nq, repeat=h // hk)
        assert_bits("grouped against the multi-head cache on repeated K / V", want, attend(*make(dev, d, h, h, Kr, Vr, lens, chunk, nq), Qd, lens)[0])
    one, _ = make(dev, d, h, hk, K, V, lens, chunk, 1)
    for r in range(nq):  # the same tiles, the same mask, the same streams
        assert_bits(f"row {r} against the one-row call", want[:, r:r + 1], attend(one, None, Qd[:, r:r + 1].contiguous(), [L - nq + 1 + r for L in lens])[0])


@pytest.mark.parametrize("paged", [False, True])
@pytest.mark.parametrize("d,chunk", [(64, 64), (128, 128)])
def test_isolation(dev, d, chunk, paged):
    """The scratch's and the cache's unwritten bytes do not reach O; nothing is written behind the scratch; an invalid length or
    table entry gives positive zeros, leaves that sequence's scratch alone and the other sequences' bits."""
    h, hk, nq = 4, 1, 5
    lens, (Q, K, V) = lens_of(nq, "mid"), inputs(d, h, hk, nq)
    Qd = torch.from_numpy(Q).to(dev)
    want, _ = attend(*make(dev, d, h, hk, K, V, lens, chunk, nq, paged), Qd, lens)  # zeroed scratch, zero bytes behind the rows
    cache, table = make(dev, d, h, hk, K, V, lens, chunk, nq, paged, fill=0x7F)  # e4m3 NaN behind ceil32(L) and in unused pages
    n = cache.decode_scratch.numel()
    cache.decode_scratch = torch.full((n + 4096,), 0xFF, dtype=torch.uint8, device=dev)
    got, scratch = attend(cache, table, Qd, lens)
    assert_bits("NaN scratch, NaN bytes behind the rows", got, want)
    assert (scratch.view(np.uint8)[n:] == 0xFF).all(), "written behind qmha_attend_decode_bytes"
    per_seq = lambda s: decode_ref.views(s, B, -(-CAP // chunk), nq, h, d)  # noqa: E731
    cache.decode_scratch.fill_(0xFF)
    got, scratch = attend(cache, table, Qd, [0, 95, 300])
    assert_bits("between two invalid lengths", got[1], want[1]), assert_zeros("lens 0", got[0]), assert_zeros("lens 300", got[2])
    assert all(np.isnan(a[[0, 2]]).all() for a in per_seq(scratch)), "an invalid sequence's scratch was written"
    if paged:
        cache.decode_scratch.fill_(0xFF)
        got, scratch = attend(cache, i32(dev, [TABLE[0], [1, PAGES, 0, 7], TABLE[2]]), Qd, lens)
        assert_zeros("a used entry outside the pool", got[1]), assert_bits("beside it", got[[0, 2]], want[[0, 2]])
        assert all(np.isnan(a[1]).all() for a in per_seq(scratch)), "an invalid sequence's scratch was written"


@pytest.mark.parametrize("d,paged", [(64, False), (128, True)])
def test_decode_loop_under_graph_replay(dev, d, paged):
    """append_tokens n = 1 + the decode call captured once on a side stream, replayed across a chunk boundary (rows 62 .. 66,
    126 .. 130; an empty slot) against the eager calls."""
    h, hk, chunk, start = 4, 2, 64, [62, 126, 0]
    Q, K, V = (torch.from_numpy(x).to(dev) for x in inputs(d, h, hk, 8))
    (graphed, table), (eager, _) = (make(dev, d, h, hk, *inputs(d, h, hk, 8)[1:], start, chunk, 1, paged) for _ in range(2))
    args = [] if table is None else [table]
    append = lambda c: c.append_paged if paged else c.append_tokens  # noqa: E731
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        qs = torch.zeros((B, 1, h * d), dtype=torch.float32, device=dev)
        ks, vs = (torch.zeros((B, 1, hk * d), dtype=torch.float32, device=dev) for _ in range(2))
        buf = torch.full((qs.numel() + 32 * h * d,), GUARD, dtype=torch.float32, device=dev)
        pos, lens, inc = i32(dev, [-1] * B), i32(dev, [0] * B), i32(dev, [1, 1, 0])
        decode = lambda c, out: (c.attend_paged_decode if paged else c.attend_decode)(qs, lens, *args, out=out)  # noqa: E731
        step = lambda: (append(graphed)(ks, vs, pos, *args), decode(graphed, buf[:qs.numel()]))  # noqa: E731
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
            append(eager)(ks, vs, pos, *args)
            want = torch.empty_like(qs)
            decode(eager, want.view(-1))
            assert bool((got[qs.numel():] == GUARD).all()), "O written past its last row"
            assert_bits(f"replay {k}", got[:qs.numel()].view(qs.shape).cpu().numpy(), want.cpu().numpy()), assert_zeros("the empty slot", want[2].cpu().numpy())
            pos.add_(inc), lens.add_(inc)
        side.synchronize()
    torch.cuda.current_stream(dev).wait_stream(side)
    assert_bits("the caches", graphed.mem.cpu().numpy(), eager.mem.cpu().numpy())


def test_compiled_module(dev):
    d, chunk, (h, hk, nq) = 64, 128, HEADS[2]
    lens, (Q, K, V) = lens_of(nq, "mid"), inputs(d, h, hk, nq)
    Qd = torch.from_numpy(Q).to(dev)
    for paged in (False, True):
        cache, table = make(dev, d, h, hk, K, V, lens, chunk, nq, paged, mod=compiled_module())
        got = cache.attend_paged_decode(Qd, i32(dev, lens), table) if paged else cache.attend_decode(Qd, i32(dev, lens))
        torch.cuda.synchronize()
        assert_bits("compiled against ctypes", got.cpu().numpy(), attend(*make(dev, d, h, hk, K, V, lens, chunk, nq, paged), Qd, lens)[0])
    from quantizedmha_amd import torch_ext
    for mod in (compiled_module(), torch_ext):
        cache = mod.GroupedKVCache(B, CAP, h * d, h, hk, FP8, str(dev))
        with pytest.raises(RuntimeError, match="max_nq \\* \\(num_heads / num_kv_heads\\) <= 32"):
            cache.enable_decode(chunk, 9)
        cache.enable_decode(chunk, 4)
        with pytest.raises(RuntimeError, match="exceed enable_decode's max_nq = 4"):
            cache.attend_decode(Qd, i32(dev, lens))
        with pytest.raises(RuntimeError, match="needs a fa_tc_fp8 cache.*attend_tokens_split"):
            mod.GroupedKVCache(B, CAP, h * d, h, hk, "fa_tc_v1a", str(dev)).enable_decode(chunk, 1)
