"""GPU tests of the fp8 cache's windowed decode call with attention sinks against its numpy restatement
(tests/decode_window_ref.py), on tests/test_gpu_decode.py's shapes: B = 3, cap 224, the pool of 64-row pages under a permuted
table.  O and every partial the combine reads are held to the restatement within FLIPS one-flip units u = 2^-4 * 2^8 * max|v| /
l plus 2^-16 max|V|, l the restatement's Ltot with the sink term in it (O) or the partial's own l."""
import functools

import numpy as np
import pytest
import torch

from tests import decode_window_ref as ref
from tests.gpu_support import GUARD, Guarded, assert_bits, assert_zeros, compiled_module, dev, i32  # noqa: F401
from tests.test_gpu_decode import B, CAP, FLIPS, FP8, PAGES, SCALES, TABLE, inputs, lens_of

pytestmark = pytest.mark.gpu
# one key per row; the left edge inside the diagonal's tile; one tile back; stage-aligned; a chunk between the edges; the cache
# covered; beyond cap.  At Nq = 8 (and 5) windows 1 and 31 leave chunk 0 without a visible key for the late rows of some lengths.
WINDOWS = (1, 31, 33, 64, 100, 224, 1000)
HEADS = [(2, 2, 1), (4, 1, 5), (8, 2, 8)]  # h, h_kv, Nq: W = 1, 20, 32 columns
EACH = pytest.mark.parametrize("d,chunk", [(64, 64), (64, 128), (128, 64), (128, 128)])
HNQ = pytest.mark.parametrize("h,hk,nq", HEADS)


def ramp(h):
    return np.linspace(-2.0, 3.0, h).astype(np.float32) if h > 1 else np.array([3.0], np.float32)


def make(dev, d, h, hk, K, V, lens, chunk, nq, paged=False, fill=0, mod=None, first=(0, 0, 0)):
    """A cache holding rows [first[b], lens[b]) of sequence b over `fill` bytes, with both decode scratches; (cache, table)."""
    from quantizedmha_amd import torch_ext
    mod = mod or torch_ext
    cache = mod.PagedKVCache(B, PAGES, 64, 4, h * d, h, hk, FP8, str(dev)) if paged else mod.GroupedKVCache(B, CAP, h * d, h, hk, FP8, str(dev))
    table = i32(dev, TABLE) if paged else None
    cache.mem.fill_(fill), cache.set_scales(*SCALES), cache.enable_tokens(), cache.enable_decode(chunk, nq), cache.enable_decode_window(chunk, 1000, nq)
    for b, (lo, L) in enumerate(zip(first, lens)):
        if L == lo:
            continue
        Kn, Vn = (torch.from_numpy(np.ascontiguousarray(np.broadcast_to(x[b, lo:L], (B, L - lo, hk * d)))).to(dev) for x in (K, V))
        pos = i32(dev, [lo if i == b else -1 for i in range(B)])
        cache.append_paged(Kn, Vn, pos, table) if paged else cache.append_tokens(Kn, Vn, pos)
    return cache, table


def attend(cache, table, Q, lens, window, sinks=None):
    """O (numpy, through the guard) and the scratch as float32 (numpy)."""
    g, s = Guarded(Q), None if sinks is None else torch.from_numpy(sinks).to(Q.device)
    if table is None:
        cache.attend_decode_window(Q, i32(Q.device, lens), window, s, out=g.buf[:g.n])
    else:
        cache.attend_paged_decode_window(Q, i32(Q.device, lens), table, window, s, out=g.buf[:g.n])
    return g.result(), cache.decode_window_scratch.cpu().numpy().view(np.float32)


@functools.lru_cache(maxsize=None)
def reference(d, h, hk, nq, lens, chunk, window, sunk):
    Q, K, V = inputs(d, h, hk, nq)
    sinks = ramp(h) if sunk else None
    O, part, Ltot, vmax = ref.decode_window(Q, K, V, lens, h, hk, SCALES, chunk, CAP, window, sinks)
    unit = FLIPS * 2.0 ** 4 * vmax, 2.0 ** -16 * float(np.abs(V).max())
    return O, part, Ltot, unit, ref.exact(Q, K, V, lens, h, hk, window, sinks)


@pytest.mark.parametrize("kind", ["edge", "mid"])
@HNQ
@EACH
def test_against_restatement_and_float64(dev, d, chunk, h, hk, nq, kind):
    lens, (Q, K, V) = lens_of(nq, kind), inputs(d, h, hk, nq)
    cache, _ = make(dev, d, h, hk, K, V, lens, chunk, nq)
    Qd, per_head = torch.from_numpy(Q).to(dev), lambda x: np.repeat(x, d, axis=-1)  # noqa: E731 -- [.., h] -> [.., h d]
    for window, sunk in ((w, s) for w in WINDOWS for s in (False, True)):
        cache.decode_window_scratch.fill_(0xFF)  # NaN: what the call leaves alone stays NaN -- all of it in the one-launch form
        got, scratch = attend(cache, None, Qd, lens, window, ramp(h) if sunk else None)
        want, (Oc, pm, pl), Ltot, (unit, fp32), exact = reference(d, h, hk, nq, lens, chunk, window, sunk)
        bound, err = per_head(unit[:, None, :] / Ltot) + fp32, np.abs(got.astype(np.float64) - want)
        print(f"window {window} sinks {sunk}: O worst err / bound = {float((err / bound).max()):.3f}")
        assert np.isfinite(got).all() and (err <= bound).all(), (window, sunk, float((err / bound).max()))
        NC = ref.chunks(CAP, nq, window, chunk)
        gOc, gm, gl = ref.views(scratch, B, NC, nq, h, d)
        assert np.array_equal(np.isnan(gl), np.isnan(pl)) and np.array_equal(np.isnan(gOc), np.isnan(Oc)) and np.array_equal(np.isnan(gm), np.isnan(pm))
        assert np.isnan(scratch[ref.layout(B, NC, nq, h, d)[1] // 4:]).all() and (NC > 1 or np.isnan(scratch).all()), "behind the call's layout"
        w = ~np.isnan(pl)
        if w.any():
            assert np.isfinite(gm[w]).all() and np.isfinite(gl[w]).all() and np.isfinite(gOc[per_head(w)]).all() and np.array_equal(gl[w] == 0, pl[w] == 0)
            perr, pbound = np.abs(gOc - Oc)[per_head(w)], (per_head(unit[:, None, None, :] / np.where(w & (pl > 0), pl, 1.0)) + fp32)[per_head(w)]
            print(f"window {window} sinks {sunk}: partials worst err / bound = {float((perr / pbound).max()):.3f}")
            assert (perr <= pbound).all(), (window, sunk, float((perr / pbound).max()))
        far, own = np.abs(got - exact).max(), np.abs(want - exact).max()  # every row: a one-key row is the window's own case
        assert far <= 1.25 * own, (window, sunk, far, own)  # the restatement's own distance from float64, never the kernel's


@HNQ
@EACH
def test_bit_identities(dev, d, chunk, h, hk, nq):
    lens, (Q, K, V) = lens_of(nq, "edge"), inputs(d, h, hk, nq)
    Qd = torch.from_numpy(Q).to(dev)
    plain, paged = make(dev, d, h, hk, K, V, lens, chunk, nq), make(dev, d, h, hk, K, V, lens, chunk, nq, paged=True)
    twin = make(dev, d, h, h, *inputs(d, h, hk, nq, repeat=h // hk)[1:], lens, chunk, nq) if hk < h else None
    for window in WINDOWS:
        want, scratch = attend(*plain, Qd, lens, window, ramp(h))
        got, pscratch = attend(*paged, Qd, lens, window, ramp(h))
        assert_bits(f"window {window}: paged against contiguous", got, want)
        assert np.array_equal(pscratch.view(np.uint32), scratch.view(np.uint32)), "paged against contiguous: the scratch"
        if twin:
            assert_bits(f"window {window}: grouped against the multi-head cache on repeated K / V", want, attend(*twin, Qd, lens, window, ramp(h))[0])
    full = torch.empty_like(Qd)
    plain[0].attend_decode(Qd, i32(dev, lens), out=full)
    for window in (224, 1000):  # window >= lens[b], no sinks, the combine form: attend_decode's chunks and its combine's order
        assert ref.chunks(CAP, nq, window, chunk) > 1
        assert_bits(f"window {window} against attend_decode", attend(*plain, Qd, lens, window)[0], full.cpu().numpy())


@pytest.mark.parametrize("paged", [False, True])
@pytest.mark.parametrize("d,chunk,window", [(64, 64, 33), (128, 64, 33), (64, 128, 32), (128, 128, 32)])
def test_isolation(dev, d, chunk, window, paged):
    """Rows before 32 t0 and behind ceil32(L), unused pages and the scratch hold NaN bytes and reach nothing; the table's
    columns behind the window hold -1; nothing is written behind the scratch, and in the one-launch form (window 32 at
    chunk_rows 128) nothing into it; an invalid length or a table entry outside the pool inside the window gives positive zeros."""
    (h, hk, nq), lens = (4, 1, 5), (33, 163, 224)
    first = tuple(32 * ref.first_tile(L, nq, window) for L in lens)  # (0, 64, 128)
    (Q, K, V), sinks = inputs(d, h, hk, nq), ramp(h)
    Qd = torch.from_numpy(Q).to(dev)
    want, _ = attend(*make(dev, d, h, hk, K, V, lens, chunk, nq, paged), Qd, lens, window, sinks)  # every row cached, zero bytes elsewhere
    cache, table = make(dev, d, h, hk, K, V, lens, chunk, nq, paged, fill=0x7F, first=first)  # e4m3 NaN wherever no swept row lies
    if paged:
        table = i32(dev, [[-1 if 64 * (c + 1) <= lo else e for c, e in enumerate(row)] for row, lo in zip(TABLE, first)])
    n = cache.decode_window_scratch.numel()
    cache.decode_window_scratch = torch.full((n + 4096,), 0xFF, dtype=torch.uint8, device=dev)
    got, scratch = attend(cache, table, Qd, lens, window, sinks)
    assert_bits("NaN scratch, NaN bytes outside the swept rows, -1 behind the window", got, want)
    direct = ref.chunks(CAP, nq, window, chunk) == 1
    assert direct == (window == 32) and (scratch.view(np.uint8)[0 if direct else n:] == 0xFF).all(), "written behind the scratch, or into it"
    got, _ = attend(cache, table, Qd, [0, 163, 300], window, sinks)
    assert_bits("between two invalid lengths", got[1], want[1]), assert_zeros("lens 0", got[0]), assert_zeros("lens 300", got[2])
    if paged:
        bad = table.clone()
        bad[1, 2] = PAGES  # rows 128 .. 191 of sequence 1: inside its window
        got, _ = attend(cache, bad, Qd, lens, window, sinks)
        assert_zeros("an entry outside the pool inside the window", got[1]), assert_bits("beside it", got[[0, 2]], want[[0, 2]])


@pytest.mark.parametrize("d,paged,chunk", [(64, False, 128), (128, True, 64)])
def test_decode_loop_under_graph_replay(dev, d, paged, chunk):
    """append n = 1 + the windowed decode call (window 33, sinks) captured once on a side stream and replayed while lens goes
    96 .. 100 (t0 0 -> 2: a stage) and 160 .. 164 (t0 2 -> 4: past a 128-row chunk), against the eager calls: the one-launch
    form at chunk_rows 128, the combine form at 64."""
    h, hk, window, start = 4, 2, 33, [95, 159, 0]
    Q, K, V = (torch.from_numpy(x).to(dev) for x in inputs(d, h, hk, 8))
    (graphed, table), (eager, _) = (make(dev, d, h, hk, *inputs(d, h, hk, 8)[1:], start, chunk, 1, paged) for _ in range(2))
    args, sinks = [] if table is None else [table], torch.from_numpy(ramp(h)).to(dev)
    append = lambda c: c.append_paged if paged else c.append_tokens  # noqa: E731
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        qs = torch.zeros((B, 1, h * d), dtype=torch.float32, device=dev)
        ks, vs = (torch.zeros((B, 1, hk * d), dtype=torch.float32, device=dev) for _ in range(2))
        buf = torch.full((qs.numel() + 32 * h * d,), GUARD, dtype=torch.float32, device=dev)
        pos, lens, inc = i32(dev, [-1] * B), i32(dev, [0] * B), i32(dev, [1, 1, 0])
        decode = lambda c, out: (c.attend_paged_decode_window if paged else c.attend_decode_window)(qs, lens, *args, window, sinks, out=out)  # noqa: E731
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
    d, chunk, (h, hk, nq) = 64, 128, HEADS[1]
    lens, (Q, K, V) = lens_of(nq, "mid"), inputs(d, h, hk, nq)
    Qd, sinks = torch.from_numpy(Q).to(dev), torch.from_numpy(ramp(h)).to(dev)
    for paged, window in ((False, 33), (True, 33), (False, 100), (True, 100)):  # the one-launch form and the combine form
        cache, table = make(dev, d, h, hk, K, V, lens, chunk, nq, paged, mod=compiled_module())
        got = cache.attend_paged_decode_window(Qd, i32(dev, lens), table, window, sinks) if paged else cache.attend_decode_window(Qd, i32(dev, lens), window, sinks)
        torch.cuda.synchronize()
        assert_bits("compiled against ctypes", got.cpu().numpy(), attend(*make(dev, d, h, hk, K, V, lens, chunk, nq, paged), Qd, lens, window, ramp(h))[0])
    from quantizedmha_amd import torch_ext
    for mod in (compiled_module(), torch_ext):
        cache = mod.GroupedKVCache(B, CAP, h * d, h, hk, FP8, str(dev))
        with pytest.raises(RuntimeError, match="call enable_decode_window"):
            cache.attend_decode_window(Qd, i32(dev, lens), 33)
        with pytest.raises(RuntimeError, match="max_nq \\* \\(num_heads / num_kv_heads\\) <= 32"):
            cache.enable_decode_window(chunk, 33, 9)
        cache.enable_decode_window(chunk, 33, nq)
        with pytest.raises(RuntimeError, match="exceeds enable_decode_window's window = 33"):
            cache.attend_decode_window(Qd, i32(dev, lens), 34)
        with pytest.raises(RuntimeError, match="sinks must be a float32 CUDA tensor of num_heads = 4"):
            cache.attend_decode_window(Qd, i32(dev, lens), 33, sinks[:3])
        with pytest.raises(RuntimeError, match="needs a fa_tc_fp8 cache.*attend_tokens_window"):
            mod.GroupedKVCache(B, CAP, h * d, h, hk, "fa_tc_v1a", str(dev)).enable_decode_window(chunk, 33, 1)
