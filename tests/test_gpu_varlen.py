"""GPU tests (MI355X) of the per-sequence entry points of the K/V cache: qmha_kv_cache_append_at and
qmha_attend_cached_varlen through torch_ext.KVCache / GroupedKVCache (ctypes) and the compiled module's classes.

The oracle is the shipped uniform path -- append / attend with one host length for the whole batch -- and every
comparison is bit for bit, so no arithmetic is restated here:
  * sequence b of attend_varlen(Q, lens) equals sequence b of attend(Q) on a uniform cache that holds the same rows
    and has len == lens[b]: the varlen kernel runs the body of the masked kernels over Rect::cached's geometry at that
    length, on byte-equal operands, over the same tiles in the same order (the Grouped unit map, which at G = 1 is
    Rect's);
  * without the mask at lens[b] < cap -- which attend cannot do -- it equals the unmasked attend of a FULL cache of
    cap == lens[b]: the same tiles 0 .. lens[b] / 32 - 1 in the same order;
  * the bytes append_at writes are those append writes at len == pos[b], and nothing else is written.
Every O is written into the head of a buffer with a sentinel-filled guard behind it.
Shapes: B = 3, cap = 224 (Gk = 7: the last stage is partial), h = 2 (grouped: h = 4 on h_kv = 2 or 1), every built
(variant, d).  A wrong per-sequence offset, tile count or slice stride moves whole tiles and fails these comparisons.
"""
import functools

import numpy as np
import pytest

from tests import gpu_support as gs
from tests import rect_ref as rr
from tests.gpu_support import (BUILT, F16, GUARD, INT8, assert_bits, assert_zeros, attend, compiled_module, dev, i32,  # noqa: F401
                               seq_slices, to_dev)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
B, CAP, NQ = 3, 224, 96
HEADS = [(2, None), (4, 2), (4, 1)]  # (h, h_kv); None: a multi-head KVCache


def new_cache(dev, variant, d, heads=HEADS[0], cap=CAP, mod=None):
    return gs.new_cache(dev, variant, B, cap, d, *heads, mod=mod)


def attend_varlen(cache, Q, lens, causal=True):
    return attend(cache, Q, causal, lens)


# ---- inputs and the uniform path's results, computed once per (variant, d, heads, dist) and left unchanged ----------
@functools.lru_cache(maxsize=None)
def host_inputs(d, heads, dist):
    """Q [B, NQ, h d], K, V [B, CAP, h_kv d].  dist "spike": `normal` with causal_ref's spike_tile (NQ, CAP) as
    sequence 0 (multi-head, h = 2: the hard case's head count)."""
    h, h_kv = heads
    seed = 7700 + d + 10 * h + (h_kv or 0)
    base = "normal" if dist == "spike" else dist
    Q = rr.inputs(NQ, CAP, h * d, B, base, seed)[0]
    _, K, V = rr.inputs(NQ, CAP, (h_kv or h) * d, B, base, seed + 1)
    if dist == "spike":
        assert heads == HEADS[0]
        q, k, v = rr.hard_inputs("spike_tile", d, NQ, CAP)
        Q, K, V = Q.copy(), K.copy(), V.copy()
        Q[0], K[0], V[0] = q[0], k[0], v[0]
    return Q, K, V


_DEV = {}


def dev_inputs(dev, d, heads, dist):
    key = (d, heads, dist)
    if key not in _DEV:
        _DEV[key] = to_dev(dev, *host_inputs(d, heads, dist))
    return _DEV[key]


_UNIFORM = {}


def uniform(dev, variant, d, heads, dist, L, Nq, causal=True):
    """The oracle: attend(Q[:, :Nq]) of a uniform cache holding rows [0, L) -- causal: of capacity CAP, len == L;
    unmasked: a full cache of cap == L.  [B, Nq, h d] (numpy)."""
    key = (variant, d, heads, dist, L, Nq, causal)
    if key not in _UNIFORM:
        Q, K, V = dev_inputs(dev, d, heads, dist)
        cache = new_cache(dev, variant, d, heads, cap=CAP if causal else L)
        cache.append(K[:, :L], V[:, :L])
        _UNIFORM[key] = attend(cache, Q[:, :Nq].contiguous(), causal=causal)
    return _UNIFORM[key]


def filled(dev, variant, d, heads, dist):
    """A cache whose CAP rows are all written (the uniform append addresses the rows append_at addresses)."""
    _, K, V = dev_inputs(dev, d, heads, dist)
    cache = new_cache(dev, variant, d, heads)
    cache.append(K, V)
    return cache


# ---- 1. placement ---------------------------------------------------------------------------------------------------
def pattern_of(cache):
    return (torch.arange(cache.mem.numel(), device=cache.mem.device) % 251).to(torch.uint8)


@pytest.mark.parametrize("heads", [HEADS[0], HEADS[1]], ids=["mha", "gqa2"])
@pytest.mark.parametrize("variant,d", BUILT)
def test_placement(dev, variant, d, heads):
    _, K, V = dev_inputs(dev, d, heads, "normal")
    n = 64
    new_k, new_v = K[:, 160:160 + n].contiguous(), V[:, 160:160 + n].contiguous()
    # (a) one row for all: the whole cache tensor equals the uniform append's
    p = 96
    a, u = new_cache(dev, variant, d, heads), new_cache(dev, variant, d, heads)
    for c in (a, u):
        c.append(K[:, :p], V[:, :p])
    a.append_at(new_k, new_v, i32(dev, [p] * B))
    u.append(new_k, new_v)
    torch.cuda.synchronize()
    assert a.len == p and u.len == p + n  # append_at leaves the host length alone
    assert torch.equal(a.mem, u.mem), "pos = [p, p, p] against append at len = p"
    # (b) a row per sequence, into a cache prefilled with a byte pattern: slice b equals that of a uniform cache
    # appended at len == pos[b] over the same pattern, and nothing else is written
    pos = [0, 64, 160]
    a = new_cache(dev, variant, d, heads)
    pattern = pattern_of(a)
    a.mem.copy_(pattern)
    a.append_at(new_k, new_v, i32(dev, pos))
    want = pattern.clone()
    for b, pb in enumerate(pos):
        u = new_cache(dev, variant, d, heads)
        if pb:
            u.append(K[:, :pb], V[:, :pb])  # only to move len to pos[b]
        u.mem.copy_(pattern)
        u.append(new_k, new_v)
        for s in seq_slices(u, b):
            want[s] = u.mem[s]
    torch.cuda.synchronize()
    assert not torch.equal(want, pattern)
    assert torch.equal(a.mem, want), "pos = [0, 64, 160]"
    # (c) invalid rows -- negative, no multiple of 32, past cap - n --: nothing is written
    a.mem.copy_(pattern)
    a.append_at(new_k, new_v, i32(dev, [-32, 48, 192]))
    torch.cuda.synchronize()
    assert torch.equal(a.mem, pattern), "invalid pos wrote to the cache"


# ---- 2. causal attend, 6. grouped caches ----------------------------------------------------------------------------
CAUSAL_CASES = [(BUILT_i, heads, dist) for BUILT_i in BUILT for heads in HEADS
                for dist in rr.DISTS + (("spike",) if heads == HEADS[0] else ())]


def case_id(v):
    if isinstance(v, tuple):
        return "-".join(str(x) for x in v)
    return str(v)


@pytest.mark.parametrize("vd,heads,dist", CAUSAL_CASES, ids=case_id)
def test_causal_attend(dev, vd, heads, dist):
    variant, d = vd
    Q = dev_inputs(dev, d, heads, dist)[0]
    cache = filled(dev, variant, d, heads, dist)
    for lens, Nq in (([224, 96, 160], 96), ([32, 160, 224], 32)):
        q = Q[:, :Nq].contiguous()
        got = attend_varlen(cache, q, i32(dev, lens))
        assert np.isfinite(got).all()
        for b, L in enumerate(lens):
            assert_bits(f"lens {lens} Nq {Nq} sequence {b}", got[b], uniform(dev, variant, d, heads, dist, L, Nq)[b])
    assert cache.len == CAP  # the host length is not touched


# ---- 3. unmasked attend at L < cap -----------------------------------------------------------------------------------
@pytest.mark.parametrize("dist", rr.DISTS)
@pytest.mark.parametrize("heads", [HEADS[0], HEADS[2]], ids=["mha", "gqa1"])
@pytest.mark.parametrize("variant,d", BUILT)
def test_unmasked_attend_below_cap(dev, variant, d, heads, dist):
    Q = dev_inputs(dev, d, heads, dist)[0]
    cache = filled(dev, variant, d, heads, dist)
    lens = [64, 224, 128]
    got = attend_varlen(cache, Q, i32(dev, lens), causal=False)
    for b, L in enumerate(lens):
        assert_bits(f"unmasked, sequence {b} at L = {L}", got[b], uniform(dev, variant, d, heads, dist, L, NQ, causal=False)[b])


# ---- 4. nothing beyond lens[b] is read --------------------------------------------------------------------------------
@pytest.mark.parametrize("causal", [True, False], ids=["causal", "full"])
@pytest.mark.parametrize("variant,d", BUILT)
def test_rows_beyond_the_length_are_never_read(dev, variant, d, causal):
    """Rows of magnitude 1e30 (inf in Kh, huge sK / sV) behind every lens[b]: the result is the clean cache's."""
    Q, K, V = dev_inputs(dev, d, HEADS[0], "normal")
    lens = [96, 160, 224] if causal else [64, 224, 128]
    dirty_k, dirty_v = K.clone(), V.clone()
    for b, L in enumerate(lens):
        dirty_k[b, L:] = 1e30
        dirty_v[b, L:] = -1e30
    dirty = new_cache(dev, variant, d)
    dirty.append(dirty_k, dirty_v)
    got = attend_varlen(dirty, Q, i32(dev, lens), causal=causal)
    assert np.isfinite(got).all()
    assert_bits("dirty tail", got, attend_varlen(filled(dev, variant, d, HEADS[0], "normal"), Q, i32(dev, lens), causal=causal))
    for b, L in enumerate(lens):
        assert_bits(f"dirty tail, sequence {b}", got[b], uniform(dev, variant, d, HEADS[0], "normal", L, NQ, causal=causal)[b])


# ---- 5. invalid and empty sequences (6.: on grouped caches too) --------------------------------------------------------
@pytest.mark.parametrize("heads", HEADS, ids=["mha", "gqa2", "gqa1"])
@pytest.mark.parametrize("variant,d", BUILT)
def test_invalid_and_empty_sequences(dev, variant, d, heads):
    Q = dev_inputs(dev, d, heads, "normal")[0]
    cache = filled(dev, variant, d, heads, "normal")
    # 0: empty; 100: no multiple of 32; 256: above cap; -32: negative; 64: below Nq = 96 (causal)
    for lens in ([0, 100, 256], [-32, 224, 64]):
        got = attend_varlen(cache, Q, i32(dev, lens))
        for b, L in enumerate(lens):
            if L == 224:
                assert_bits(f"lens {lens}: the valid sequence {b}", got[b], uniform(dev, variant, d, heads, "normal", L, NQ)[b])
            else:
                assert_zeros(f"lens {lens}: sequence {b}", got[b])


# ---- 7. graph replay with advancing lengths ---------------------------------------------------------------------------
@pytest.mark.parametrize("variant,d", [(INT8, 64), (F16, 128)])
def test_graph_replay_follows_the_lengths(dev, variant, d):
    """One append_at(n = 32) and one attend_varlen(Nq = 32) captured once on a side stream (single stream, linear) over
    static tensors; three replays, between which new K, V, Q are copied in and pos / lens advance by 32 on that stream.
    Sequences 0 and 1 start at 32 and 96 rows; sequence 2 is an empty slot (pos < 0, lens = 0) that is skipped."""
    Q, K, V = dev_inputs(dev, d, HEADS[0], "normal")
    start, steps, n = [32, 96], 3, 32
    new = [(Q[:, 32 * k:32 * k + n].contiguous(), K[:, 128 + 32 * k:128 + 32 * k + n].contiguous(),
            V[:, 128 + 32 * k:128 + 32 * k + n].contiguous()) for k in range(steps)]
    # the eager uniform path, per sequence: its prefill rows, then the steps' rows, attended with the step's queries
    want = []
    for b, L0 in enumerate(start):
        u = new_cache(dev, variant, d)
        u.append(K[:, :L0], V[:, :L0])
        outs = []
        for q, k, v in new:
            u.append(k, v)
            outs.append(attend(u, q)[b])
        want.append(outs)
    cache = new_cache(dev, variant, d)
    cache.append(K[:, :96], V[:, :96])  # rows [32, 96) of sequence 0 are overwritten by its steps
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    got = []
    with torch.cuda.stream(side):
        qs, ks, vs = (torch.zeros_like(x) for x in new[0])
        buf = torch.full((qs.numel() + 32 * qs.shape[-1],), GUARD, dtype=torch.float32, device=dev)
        pos, lens = i32(dev, [-32] * B), i32(dev, [0] * B)
        cache.append_at(ks, vs, pos)  # both kernels once before the capture; every sequence invalid: nothing is placed
        cache.attend_varlen(qs, lens, out=buf[:qs.numel()])
        pos.copy_(i32(dev, start + [-32]))
        lens.copy_(i32(dev, [L + n for L in start] + [0]))
        inc = i32(dev, [n, n, 0])
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            cache.append_at(ks, vs, pos)
            cache.attend_varlen(qs, lens, out=buf[:qs.numel()])
        for q, k, v in new:
            qs.copy_(q), ks.copy_(k), vs.copy_(v)
            graph.replay()
            got.append(buf.clone())
            pos.add_(inc), lens.add_(inc)
        side.synchronize()
    torch.cuda.current_stream(dev).wait_stream(side)
    assert pos.tolist() == [32 + 96, 96 + 96, -32] and cache.len == 96
    for k, g in enumerate(got):
        g = g.cpu().numpy()
        assert (g[qs.numel():] == GUARD).all(), "O written past its last row"
        o = g[:qs.numel()].reshape(qs.shape)
        for b in range(2):
            assert_bits(f"replay {k} sequence {b}", o[b], want[b][k])
        assert (o[2] == 0.0).all(), f"replay {k}: the empty slot"
    assert not np.array_equal(got[0].cpu().numpy(), got[1].cpu().numpy())


# ---- 8. both bindings -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("heads", [HEADS[0], HEADS[1]], ids=["mha", "gqa2"])
@pytest.mark.parametrize("variant,d", [(INT8, 64), (F16, 64)])
def test_compiled_binding_gives_the_same_bytes(dev, variant, d, heads):
    Q, K, V = dev_inputs(dev, d, heads, "normal")
    pos, lens = i32(dev, [0, 64, -32]), i32(dev, [96, 160, 0])
    caches = [new_cache(dev, variant, d, heads), new_cache(dev, variant, d, heads, mod=compiled_module())]
    outs = []
    for c in caches:
        c.append(K[:, :64], V[:, :64])
        c.append_at(K[:, 64:160].contiguous(), V[:, 64:160].contiguous(), pos)
        outs.append(attend_varlen(c, Q, lens))
        plain = c.attend_varlen(Q, lens)  # without out: a tensor shaped like Q
        torch.cuda.synchronize()
        assert plain.shape == Q.shape and np.array_equal(plain.cpu().numpy(), outs[-1])
    assert torch.equal(caches[0].mem, caches[1].mem)
    assert_bits("compiled against ctypes", outs[1], outs[0])
    assert (outs[0][2] == 0.0).all() and np.abs(outs[0][:2]).max() > 0.0
    for c in caches:  # dtype, shape and device are checked before the call
        with pytest.raises(RuntimeError, match="int32"):
            c.attend_varlen(Q, lens.to(torch.int64))
        with pytest.raises(RuntimeError, match="shape"):
            c.attend_varlen(Q, lens[:2])
        with pytest.raises(RuntimeError, match="CUDA"):
            c.append_at(K[:, :32].contiguous(), V[:, :32].contiguous(), pos.cpu())
