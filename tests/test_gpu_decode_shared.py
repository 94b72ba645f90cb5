"""GPU tests of the fp8 cache's shared-prefix decode call.  The reference is attend_decode / attend_paged_decode
on a cache in which every sequence holds its own copy of the prefix rows: the shared call gives its bits.

cap 320, prefix_rows 128 (the pool: 5 columns of 64-row pages under a permuted table).  The shared cache holds e4m3 NaN bytes
wherever the call may not read: sequence b > 0's rows below the prefix's end, and behind every sequence's last row; on a pool the
table columns of those rows are -1.  Every batch has a sequence with lens - Nq == prefix_rows, a ragged mid-tile length, one at
cap and one with lens - Nq < prefix_rows, which comes back as zeros."""
import functools

import numpy as np
import pytest
import torch

from tests import decode_ref
from tests import rect_ref as rr
from tests.gpu_support import Guarded, assert_bits, assert_zeros, compiled_module, dev, i32  # noqa: F401
from tests.test_gpu_decode import FLIPS, FP8, SCALES

pytestmark = pytest.mark.gpu
CAP, P, PAGE = 320, 128, 64
EACH = pytest.mark.parametrize("d,chunk", [(64, 64), (64, 128), (128, 64), (128, 128)])
# B, h, h_kv, Nq: three columns in one block; W = 20, blocks straddle sequences; 80 columns, two groups and a remainder
SHAPES = pytest.mark.parametrize("B,h,hk,nq", [(3, 2, 2, 1), (3, 4, 1, 5), (5, 8, 2, 4)])
PAGED = pytest.mark.parametrize("paged", [False, True])


def lens_of(B, nq):
    """P + nq sits mid-tile as well; the last but one (B 5) or the last is left out."""
    return (P + nq, CAP, P + nq - 1) if B == 3 else (213, P + nq, CAP, P + nq - 1, 277)


def table_of(B):
    return np.random.default_rng(3).permutation(B * (CAP // PAGE)).reshape(B, CAP // PAGE).astype(np.int32)  # page B * 5 is in no sequence


@functools.lru_cache(maxsize=None)
def inputs(d, B, h, hk, nq):
    """Q [B, nq, h d]; K, V [B, CAP, hk d] with sequence 0's first P rows in every sequence."""
    Q, K, V = rr.inputs(nq, CAP, h * d, B, "normal", 21)[0], *rr.inputs(1, CAP, hk * d, B, "normal", 22)[1:]
    K[:, :P], V[:, :P] = K[:1, :P], V[:1, :P]
    return Q, K, V


def make(dev, d, B, h, hk, K, V, rows, chunk, nq, paged, shared, mod=None):
    """A cache over e4m3 NaN bytes with rows[b] rows of sequence b -- shared: of b > 0 only those from row P on, and sequence 0's
    prefix whatever rows[0] is -- and the decode scratch for nq rows; (cache, the table to attend with)."""
    from quantizedmha_amd import torch_ext
    mod, full = mod or torch_ext, table_of(B)
    cache = mod.PagedKVCache(B, B * 5 + 1, PAGE, 5, h * d, h, hk, FP8, str(dev)) if paged else mod.GroupedKVCache(B, CAP, h * d, h, hk, FP8, str(dev))
    cache.mem.fill_(0x7F), cache.set_scales(*SCALES), cache.enable_tokens(), cache.enable_decode(chunk, nq)
    for b, L in enumerate(rows):
        lo, hi = (P if shared and b else 0), (max(L, P) if shared and not b else L)
        if hi <= lo:
            continue
        Kn, Vn = (torch.from_numpy(np.ascontiguousarray(np.broadcast_to(x[b, lo:hi], (B, hi - lo, hk * d)))).to(dev) for x in (K, V))
        pos = i32(dev, [lo if i == b else -1 for i in range(B)])
        cache.append_paged(Kn, Vn, pos, i32(dev, full)) if paged else cache.append_tokens(Kn, Vn, pos)
    if shared:
        full[1:, :P // PAGE] = -1  # the columns that hold only prefix rows
    return cache, (i32(dev, full) if paged else None)


def attend(cache, table, Q, lens, shared):
    """O (numpy, through the guard) of the shared call or of the decode call."""
    g, lens = Guarded(Q), i32(Q.device, lens)
    if shared:
        cache.attend_decode_shared(Q, lens, P, out=g.buf[:g.n]) if table is None else cache.attend_paged_decode_shared(Q, lens, table, P, out=g.buf[:g.n])
    else:
        cache.attend_decode(Q, lens, out=g.buf[:g.n]) if table is None else cache.attend_paged_decode(Q, lens, table, out=g.buf[:g.n])
    return g.result()


@functools.lru_cache(maxsize=None)
def reference(d, B, h, hk, nq, chunk):
    lens, (Q, K, V) = lens_of(B, nq), inputs(d, B, h, hk, nq)
    O, _, Ltot, vmax = decode_ref.decode(Q, K, V, lens, h, hk, SCALES, chunk, CAP)
    bound = np.repeat(FLIPS * 2.0 ** 4 * vmax[:, None, :] / Ltot, d, axis=-1) + 2.0 ** -16 * float(np.abs(V).max())
    return O, bound, decode_ref.exact(Q, K, V, lens, h, hk)


@PAGED
@SHAPES
@EACH
def test_bits_against_the_unshared_call(dev, d, chunk, B, h, hk, nq, paged):
    lens, (Q, K, V) = lens_of(B, nq), inputs(d, B, h, hk, nq)
    Qd, ok = torch.from_numpy(Q).to(dev), np.array([L - nq >= P for L in lens])
    want = attend(*make(dev, d, B, h, hk, K, V, lens, chunk, nq, paged, False), Qd, lens, False)
    got = attend(*make(dev, d, B, h, hk, K, V, lens, chunk, nq, paged, True), Qd, lens, True)
    assert_bits("shared against a copy of the prefix in every sequence", got[ok], want[ok]), assert_zeros("lens - Nq < prefix_rows", got[~ok])
    ref, bound, exact = reference(d, B, h, hk, nq, chunk)  # test_gpu_decode.py's bounds for attend_decode
    err = np.abs(got.astype(np.float64) - ref)[ok]
    print(f"O: worst err / bound = {float((err / bound[ok]).max()):.3f}")
    assert (err <= bound[ok]).all(), float((err / bound[ok]).max())
    far, own = np.abs(got - exact)[ok].max(), np.abs(ref - exact)[ok].max()
    assert far <= 1.25 * own, (far, own)  # the restatement's own distance from float64, never the kernel's


@PAGED
@pytest.mark.parametrize("d,chunk", [(64, 64), (128, 128)])
def test_isolation(dev, d, chunk, paged):
    """Nothing is written outside O's rows or behind qmha_attend_decode_bytes; NaN scratch does not reach O; a sequence that is
    left out gives positive zeros and leaves the others' bits; a prefix entry outside the pool gives zeros for all."""
    B, h, hk, nq = 5, 8, 2, 4
    lens, (Q, K, V) = lens_of(B, nq), inputs(d, B, h, hk, nq)
    Qd = torch.from_numpy(Q).to(dev)
    cache, table = make(dev, d, B, h, hk, K, V, lens, chunk, nq, paged, True)
    want = attend(cache, table, Qd, lens, True)  # zeroed scratch
    n = cache.decode_scratch.numel()
    cache.decode_scratch = torch.full((n + 4096,), 0xFF, dtype=torch.uint8, device=dev)
    assert_bits("NaN scratch", attend(cache, table, Qd, lens, True), want)
    assert bool((cache.decode_scratch[n:] == 0xFF).all()), "written behind qmha_attend_decode_bytes"
    got = attend(cache, table, Qd, [100, P + nq, 0, CAP + 1, 277], True)  # sequence 0 short of the prefix: its rows are still the prefix
    assert_bits("beside sequences that are left out", got[[1, 4]], want[[1, 4]]), assert_zeros("lens 100, 0, cap + 1", got[[0, 2, 3]])
    if paged:
        bad = table.clone()
        bad[4, 3] = B * 5 + 1  # holds rows 192 .. 255 of sequence 4
        got = attend(cache, bad, Qd, lens, True)
        assert_zeros("a used entry outside the pool", got[4]), assert_bits("beside it", got[:4], want[:4])
        bad = table.clone()
        bad[0, 1] = -1
        assert_zeros("a prefix entry outside the pool", attend(cache, bad, Qd, lens, True))


def test_graph_replay(dev):
    """One step captured once on a side stream, replayed with lens advanced in device memory, against the eager call."""
    d, chunk, (B, h, hk, nq), paged = 64, 64, (3, 4, 1, 5), True
    Q, K, V = inputs(d, B, h, hk, nq)
    cache, table = make(dev, d, B, h, hk, K, V, (200, CAP, 150), chunk, nq, paged, True)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        Qd, lens = torch.from_numpy(Q).to(dev), i32(dev, [190, CAP - 2, P + nq - 2])  # the last: left out until the third step
        out, want = torch.zeros_like(Qd), torch.zeros_like(Qd)
        cache.attend_paged_decode_shared(Qd, lens, table, P, out=out.view(-1))  # once before the capture
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            cache.attend_paged_decode_shared(Qd, lens, table, P, out=out.view(-1))
        for k in range(3):
            out.fill_(7.25)
            graph.replay()
            got = out.clone()
            cache.attend_paged_decode_shared(Qd, lens, table, P, out=want.view(-1))
            assert_bits(f"replay {k}", got.cpu().numpy(), want.cpu().numpy())
            assert bool((got[2] == 0).all()) == (k < 2)
            lens.add_(1)
        side.synchronize()
    torch.cuda.current_stream(dev).wait_stream(side)


def test_compiled_module(dev):
    d, chunk, (B, h, hk, nq) = 64, 128, (3, 4, 1, 5)
    lens, (Q, K, V) = lens_of(B, nq), inputs(d, B, h, hk, nq)
    Qd = torch.from_numpy(Q).to(dev)
    from quantizedmha_amd import torch_ext
    for paged in (False, True):
        got, want = (attend(*make(dev, d, B, h, hk, K, V, lens, chunk, nq, paged, True, mod=mod), Qd, lens, True) for mod in (compiled_module(), torch_ext))
        assert_bits("compiled against ctypes", got, want)
    for mod in (compiled_module(), torch_ext):
        cache = mod.GroupedKVCache(B, CAP, h * d, h, hk, FP8, str(dev))
        with pytest.raises(RuntimeError, match="call enable_decode\\(chunk_rows\\) first"):
            cache.attend_decode_shared(Qd, i32(dev, lens), P)
        cache.enable_decode(chunk, nq)
        with pytest.raises(RuntimeError, match="prefix_rows = 192 must be a multiple of chunk_rows = 128.*attend_decode"):
            cache.attend_decode_shared(Qd, i32(dev, lens), 192)
