"""GPU tests of the fp8 cache's windowed prefill call with attention sinks against its numpy restatement
(tests/prefill_window_ref.py), on tests/test_gpu_decode.py's cache: B = 3, cap 224, the pool of 64-row pages under a permuted
table.  O is held to the restatement within FLIPS one-flip units u_r = 2^-4 * 2^8 * max|v| / l_r plus 2^-16 max|V|
(DESIGN.md 24.5), l_r the restatement's row sum with the sink term in it."""
import functools

import numpy as np
import pytest
import torch

from tests import decode_window_ref as dwr
from tests import prefill_window_ref as ref
from tests.gpu_support import GUARD, Guarded, assert_bits, assert_zeros, compiled_module, dev, i32  # noqa: F401
from tests.test_gpu_decode import B, CAP, FLIPS, FP8, PAGES, SCALES, TABLE, inputs
from tests.test_gpu_decode_window import ramp

pytestmark = pytest.mark.gpu
# one key per row; the left edge inside the diagonal's tile; one tile back; stage-aligned; between two stages; beyond cap
WINDOWS = (1, 31, 33, 64, 100, 1000)
# h, h_kv, Nq: one row; G = 4, two query groups of four heads; G = 4 over three or four groups; G = 1 with five query groups --
# staggered bands inside a workgroup, and a second workgroup whose first stage is not stage 0
HEADS = [(2, 2, 1), (4, 1, 33), (8, 2, 70), (2, 2, 100)]
HNQ = pytest.mark.parametrize("h,hk,nq", HEADS)
EACH_D = pytest.mark.parametrize("d", [64, 128])


def lens_of(nq, kind):
    return (nq, max(nq, 165), 224) if kind == "edge" else (max(nq, 33), max(nq, 95), 193)


def first_row(L, nq, window):
    """32 t0_min: the first staged row of a sequence -- the two-tile stage of the first tile of query group 0 of the padded
    block, whose first row ends at key floor32(L - nq)."""
    return max(0, (L - nq) // 32 * 32 - window + 1) // 64 * 64


def make(dev, d, h, hk, K, V, lens, paged=False, fill=0, mod=None, first=(0, 0, 0)):
    """A cache holding rows [first[b], lens[b]) of sequence b over `fill` bytes; (cache, table)."""
    from quantizedmha_amd import torch_ext
    mod = mod or torch_ext
    cache = mod.PagedKVCache(B, PAGES, 64, 4, h * d, h, hk, FP8, str(dev)) if paged else mod.GroupedKVCache(B, CAP, h * d, h, hk, FP8, str(dev))
    table = i32(dev, TABLE) if paged else None
    cache.mem.fill_(fill), cache.set_scales(*SCALES), cache.enable_tokens()
    for b, (lo, L) in enumerate(zip(first, lens)):
        Kn, Vn = (torch.from_numpy(np.ascontiguousarray(np.broadcast_to(x[b, lo:L], (B, L - lo, hk * d)))).to(dev) for x in (K, V))
        pos = i32(dev, [lo if i == b else -1 for i in range(B)])
        cache.append_paged(Kn, Vn, pos, table) if paged else cache.append_tokens(Kn, Vn, pos)
    return cache, table


def attend(cache, table, Q, lens, window, sinks=None):
    g, s = Guarded(Q), None if sinks is None else torch.from_numpy(sinks).to(Q.device)
    if table is None:
        cache.attend_prefill_window(Q, i32(Q.device, lens), window, s, out=g.buf[:g.n])
    else:
        cache.attend_paged_prefill_window(Q, i32(Q.device, lens), table, window, s, out=g.buf[:g.n])
    return g.result()


def banded(dev, lens, nq, window):
    """TABLE with every column wholly behind a sequence's band set to -1."""
    return i32(dev, [[-1 if 64 * (c + 1) <= first_row(L, nq, window) else e for c, e in enumerate(row)] for row, L in zip(TABLE, lens)])


@functools.lru_cache(maxsize=None)
def reference(d, h, hk, nq, lens, window, sunk):
    Q, K, V = inputs(d, h, hk, nq)
    sinks = ramp(h) if sunk else None
    O, Ltot, vmax = ref.prefill_window(Q, K, V, lens, h, hk, SCALES, CAP, window, sinks)
    bound = np.repeat(FLIPS * 2.0 ** 4 * vmax[:, None, :] / Ltot, d, axis=-1) + 2.0 ** -16 * float(np.abs(V).max())
    return O, bound, dwr.exact(Q, K, V, lens, h, hk, window, sinks)


@pytest.mark.parametrize("kind", ["edge", "mid"])
@HNQ
@EACH_D
def test_against_restatement_and_float64(dev, d, h, hk, nq, kind):
    lens, (Q, K, V) = lens_of(nq, kind), inputs(d, h, hk, nq)
    cache, _ = make(dev, d, h, hk, K, V, lens)
    Qd = torch.from_numpy(Q).to(dev)
    for window, sunk in ((w, s) for w in WINDOWS for s in (False, True)):
        got = attend(cache, None, Qd, lens, window, ramp(h) if sunk else None)
        want, bound, exact = reference(d, h, hk, nq, lens, window, sunk)
        err = np.abs(got.astype(np.float64) - want)
        print(f"window {window} sinks {sunk}: O worst err / bound = {float((err / bound).max()):.3f}")
        assert np.isfinite(got).all() and (err <= bound).all(), (window, sunk, float((err / bound).max()))
        far, own = np.abs(got - exact).max(), np.abs(want - exact).max()
        assert far <= 1.25 * own, (window, sunk, far, own)  # the restatement's own distance from float64, never the kernel's


@HNQ
@EACH_D
def test_bit_identities(dev, d, h, hk, nq):
    lens, (Q, K, V) = lens_of(nq, "edge"), inputs(d, h, hk, nq)
    Qd = torch.from_numpy(Q).to(dev)
    plain, (pool, _) = make(dev, d, h, hk, K, V, lens), make(dev, d, h, hk, K, V, lens, paged=True)
    twin = make(dev, d, h, h, *inputs(d, h, hk, nq, repeat=h // hk)[1:], lens) if hk < h else None
    for window in WINDOWS:
        want = attend(*plain, Qd, lens, window, ramp(h))
        assert_bits(f"window {window}: paged, -1 behind the band, against contiguous", attend(pool, banded(dev, lens, nq, window), Qd, lens, window, ramp(h)), want)
        if twin:
            assert_bits(f"window {window}: grouped against the multi-head cache on repeated K / V", want, attend(*twin, Qd, lens, window, ramp(h)))
    g = Guarded(Qd)
    plain[0].attend_tokens(Qd, i32(dev, lens), out=g.buf[:g.n])
    assert_bits("window 1000, no sinks, against attend_tokens", attend(*plain, Qd, lens, 1000), g.result())


@pytest.mark.parametrize("paged", [False, True])
@EACH_D
def test_isolation(dev, d, paged):
    """Rows before 32 t0_min and behind ceil32(L) and unused pages hold NaN bytes and reach nothing; the table's columns behind
    the band hold -1; an invalid length or a table entry outside the pool among the read columns gives positive zeros."""
    (h, hk, nq), lens, window = HEADS[1], (40, 165, 224), 33
    first = tuple(first_row(L, nq, window) for L in lens)
    assert first == (0, 64, 128)
    (Q, K, V), sinks = inputs(d, h, hk, nq), ramp(h)
    Qd = torch.from_numpy(Q).to(dev)
    want = attend(*make(dev, d, h, hk, K, V, lens, paged), Qd, lens, window, sinks)  # every row cached, zero bytes elsewhere
    cache, table = make(dev, d, h, hk, K, V, lens, paged, fill=0x7F, first=first)  # e4m3 NaN wherever no staged row lies
    table = banded(dev, lens, nq, window) if paged else None
    assert_bits("NaN bytes outside the staged rows, -1 behind the band", attend(cache, table, Qd, lens, window, sinks), want)
    got = attend(cache, table, Qd, [32, 165, 300], window, sinks)  # through the guard: nothing is written behind O
    assert_bits("between two invalid lengths", got[1], want[1]), assert_zeros("lens 32 < Nq", got[0]), assert_zeros("lens 300", got[2])
    if paged:
        bad = table.clone()
        bad[1, 1] = PAGES  # rows 64 .. 127 of sequence 1: inside its band's stages
        got = attend(cache, bad, Qd, lens, window, sinks)
        assert_zeros("an entry outside the pool among the read columns", got[1]), assert_bits("beside it", got[[0, 2]], want[[0, 2]])


def test_compiled_module(dev):
    d, (h, hk, nq), window = 64, HEADS[2], 100
    lens, (Q, K, V) = lens_of(nq, "mid"), inputs(d, h, hk, nq)
    Qd, sinks = torch.from_numpy(Q).to(dev), torch.from_numpy(ramp(h)).to(dev)
    for paged in (False, True):
        cache, table = make(dev, d, h, hk, K, V, lens, paged, mod=compiled_module())
        got = cache.attend_paged_prefill_window(Qd, i32(dev, lens), table, window, sinks) if paged else cache.attend_prefill_window(Qd, i32(dev, lens), window, sinks)
        torch.cuda.synchronize()
        assert_bits("compiled against ctypes", got.cpu().numpy(), attend(*make(dev, d, h, hk, K, V, lens, paged), Qd, lens, window, ramp(h)))
    with pytest.raises(RuntimeError, match="fa_tc_fp8 cache only.*attend_tokens_window"):
        compiled_module().GroupedKVCache(B, CAP, h * d, h, hk, "fa_tc_v1a", str(dev)).attend_prefill_window(Qd, i32(dev, lens), window)


@pytest.mark.parametrize("d,paged", [(64, False), (128, True)])
def test_graph_replay_across_a_stage(dev, d, paged):
    """The call captured once on a side stream and replayed while lens goes 99 .. 103 (t0 0 -> 2) and 163 .. 167 (2 -> 4) beside
    an invalid slot, against the eager call."""
    (h, hk, nq), window, start = (4, 2, 5), 33, [99, 163, 0]
    Q, K, V = inputs(d, h, hk, nq)
    cache, table = make(dev, d, h, hk, K, V, (CAP, CAP, CAP), paged)
    args, Qd, sinks = [] if table is None else [table], torch.from_numpy(Q).to(dev), torch.from_numpy(ramp(h)).to(dev)
    call = cache.attend_paged_prefill_window if paged else cache.attend_prefill_window
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        buf = torch.full((Qd.numel() + 32 * h * d,), GUARD, dtype=torch.float32, device=dev)
        lens, inc = i32(dev, [0] * B), i32(dev, [1, 1, 0])
        call(Qd, lens, *args, window, sinks, out=buf[:Qd.numel()])  # once before the capture: every sequence invalid
        lens.copy_(i32(dev, start))
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            call(Qd, lens, *args, window, sinks, out=buf[:Qd.numel()])
        for k in range(5):
            graph.replay()
            got, want = buf.clone(), torch.empty_like(Qd)
            call(Qd, lens, *args, window, sinks, out=want.view(-1))
            assert bool((got[Qd.numel():] == GUARD).all()), "O written past its last row"
            assert_bits(f"replay {k}", got[:Qd.numel()].view(Qd.shape).cpu().numpy(), want.cpu().numpy()), assert_zeros("the empty slot", want[2].cpu().numpy())
            lens.add_(inc)
        side.synchronize()
    torch.cuda.current_stream(dev).wait_stream(side)
