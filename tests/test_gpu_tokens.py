"""GPU tests (MI355X) of the token-granular entry points of the K/V cache: qmha_kv_cache_append_tokens and
qmha_attend_cached_tokens through torch_ext.KVCache / GroupedKVCache (ctypes) and the compiled module's classes.

The contract defines a ragged call as the existing call on zero-padded operands, so the yardstick is the existing path
and every comparison is bit for bit:
  * after append_tokens the cache tensor equals that of a fresh cache given the same rows, zero-padded to ceil32, through
    append_at -- every byte of it, from one byte pattern, so nothing outside the touched groups is written either;
  * sequence b of attend_tokens(Q, lens) equals rows [s, s + Nq) of attend_varlen on a zero [Nq', h d] block holding Q
    there, at ceil32(lens[b]), over the same cache (s = (lens[b] - Nq) mod 32, Nq' = ceil32(s + Nq)).
Every O is written into the head of a buffer with a sentinel-filled guard behind it.
Shapes: B = 3, cap = 224 (Gk = 7: the last stage is partial), h = 2 (grouped: h = 4 on h_kv = 2 or 1), every built
(variant, d).
"""
import functools

import numpy as np
import pytest

from tests import gpu_support as gs
from tests import rect_ref as rr
from tests.gpu_support import (BUILT, F16, GUARD, INT8, Guarded, assert_bits, assert_zeros, attend, compiled_module, dev,  # noqa: F401
                               i32, to_dev)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
B, CAP, NQ = 3, 224, 64
HEADS = [(2, None), (4, 2), (4, 1)]  # (h, h_kv); None: a multi-head KVCache
HEAD_IDS = ["mha", "gqa2", "gqa1"]


def ceil32(x):
    return -(-x // 32) * 32


@functools.lru_cache(maxsize=None)
def host_inputs(d, heads, dist="normal"):
    """Q [B, NQ, h d], K, V [B, CAP, h_kv d]."""
    h, h_kv = heads
    seed = 8800 + d + 10 * h + (h_kv or 0)
    Q = rr.inputs(NQ, CAP, h * d, B, dist, seed)[0]
    _, K, V = rr.inputs(NQ, CAP, (h_kv or h) * d, B, dist, seed + 1)
    return Q, K, V


_DEV = {}


def dev_inputs(dev, d, heads, dist="normal"):
    key = (d, heads, dist)
    if key not in _DEV:
        _DEV[key] = to_dev(dev, *host_inputs(d, heads, dist))
    return _DEV[key]


def new_cache(dev, variant, d, heads=HEADS[0], mod=None, tokens=True):
    c = gs.new_cache(dev, variant, B, CAP, d, *heads, mod=mod)
    if tokens:
        c.enable_tokens()
    return c


def pattern_of(cache):
    return (torch.arange(cache.mem.numel(), device=cache.mem.device) % 251).to(torch.uint8)


def padded_cache(dev, variant, d, heads, K, V, Ls, pattern=True):
    """The yardstick: a fresh cache (over the byte pattern) that holds rows [0, Ls[b]) of K[b], V[b] zero-padded to
    ceil32(Ls[b]), written a 32-row group at a time through append_at; a sequence with no rows in a group is left out
    of that call (pos < 0)."""
    c = new_cache(dev, variant, d, heads, tokens=False)
    if pattern:
        c.mem.copy_(pattern_of(c))
    Kp, Vp = K.clone(), V.clone()
    for b, L in enumerate(Ls):
        Kp[b, L:], Vp[b, L:] = 0.0, 0.0
    for g in range(CAP // 32):
        pos = [32 * g if 32 * g < L else -32 for L in Ls]
        if max(pos) >= 0:
            c.append_at(Kp[:, 32 * g:32 * g + 32].contiguous(), Vp[:, 32 * g:32 * g + 32].contiguous(), i32(dev, pos))
    return c


def rows_at(X, pos, n):
    """[B, n, w]: sequence b's rows [pos[b], pos[b] + n) of X (rows [0, n) where pos[b] is invalid)."""
    return torch.stack([X[b, p:p + n] if 0 <= p <= CAP - n else X[b, :n] for b, p in enumerate(pos)]).contiguous()


def append_tokens_at(cache, K, V, pos, n):
    cache.append_tokens(rows_at(K, pos, n), rows_at(V, pos, n), i32(K.device, pos))


def attend_tokens(cache, Q, lens):
    g = Guarded(Q)
    cache.attend_tokens(Q, lens, out=g.buf[:g.n])
    return g.result()


def padded_attend(dev, cache, Q, b, L):
    """Rows [s, s + Nq) of sequence b of attend_varlen on the zero [B, Nq', h d] block that holds Q[b] at rows
    [s, s + Nq), at ceil32(L), the other sequences left out (lens 0): [Nq, h d] (numpy)."""
    Nq = Q.shape[1]
    s = (L - Nq) % 32
    Qp = torch.zeros((B, ceil32(s + Nq), Q.shape[2]), dtype=torch.float32, device=dev)
    Qp[b, s:s + Nq] = Q[b]
    lens = [ceil32(L) if i == b else 0 for i in range(B)]
    return attend(cache, Qp, True, i32(dev, lens))[b, s:s + Nq]


def check_attend(dev, cache, Q, lens, label, yard=None):
    """attend_tokens(Q, lens) on `cache` against the padded path on `yard` (default: the same cache), per sequence; an
    invalid length (outside [Nq, CAP]) gives positive zeros."""
    got = attend_tokens(cache, Q, i32(dev, lens))
    for b, L in enumerate(lens):
        if Q.shape[1] <= L <= CAP:
            assert_bits(f"{label} lens {lens} Nq {Q.shape[1]} sequence {b}", got[b], padded_attend(dev, yard or cache, Q, b, L))
            assert np.abs(got[b]).max() > 0.0
        else:
            assert_zeros(f"{label} lens {lens} Nq {Q.shape[1]} sequence {b} (invalid)", got[b])
    return got


def filled(dev, variant, d, heads, K=None, V=None):
    """A cache whose CAP rows are all written by the uniform append."""
    _, K0, V0 = dev_inputs(dev, d, heads)
    c = new_cache(dev, variant, d, heads)
    c.append(K0 if K is None else K, V0 if V is None else V)
    return c


# ---- 1. append (5.: on grouped caches too) ----------------------------------------------------------------------------
@pytest.mark.parametrize("heads", [HEADS[0], HEADS[1]], ids=HEAD_IDS[:2])
@pytest.mark.parametrize("variant,d", BUILT)
def test_append_tokens_writes_the_padded_bytes(dev, variant, d, heads):
    _, K, V = dev_inputs(dev, d, heads)
    pos = [0, 31, 64]
    for n in (1, 7, 33, 70):
        a = new_cache(dev, variant, d, heads)
        a.mem.copy_(pattern_of(a))
        # what lies ahead of pos[b]: 31 rows of sequence 1 built token-wise from row 0 (they fill the tail), two full
        # groups of sequence 2
        append_tokens_at(a, K, V, [-1, 0, -1], 31)
        a.append_at(K[:, :64].contiguous(), V[:, :64].contiguous(), i32(dev, [-32, -32, 0]))
        append_tokens_at(a, K, V, pos, n)
        want = padded_cache(dev, variant, d, heads, K, V, [p + n for p in pos])
        torch.cuda.synchronize()
        assert a.len == 0  # the host length is not touched
        assert not torch.equal(want.mem, pattern_of(want))
        assert torch.equal(a.mem, want.mem), f"n = {n} at pos = {pos}"


@pytest.mark.parametrize("variant,d", BUILT)
def test_single_token_appends_cross_group_boundaries(dev, variant, d):
    """30 rows, then one row at a time up to 70 (sequence 2: 96 rows further on, behind three groups placed by append_at):
    after every call the whole cache tensor is the padded yardstick's."""
    _, K, V = dev_inputs(dev, d, HEADS[0])
    off = [0, 0, 96]
    a = new_cache(dev, variant, d)
    a.mem.copy_(pattern_of(a))
    a.append_at(K[:, :96].contiguous(), V[:, :96].contiguous(), i32(dev, [-32, -32, 0]))
    append_tokens_at(a, K, V, off, 30)
    for L in range(30, 70):
        append_tokens_at(a, K, V, [o + L for o in off], 1)
        want = padded_cache(dev, variant, d, HEADS[0], K, V, [o + L + 1 for o in off])
        assert torch.equal(a.mem, want.mem), f"after the row at {L}"


@pytest.mark.parametrize("heads", [HEADS[0], HEADS[2]], ids=["mha", "gqa1"])
@pytest.mark.parametrize("variant,d", BUILT)
def test_invalid_pos_writes_nothing(dev, variant, d, heads):
    _, K, V = dev_inputs(dev, d, heads)
    a = new_cache(dev, variant, d, heads)
    a.mem.copy_(pattern_of(a))
    a.append_at(K[:, :96].contiguous(), V[:, :96].contiguous(), i32(dev, [-32, -32, 0]))
    append_tokens_at(a, K, V, [-1, -1, 96], 4)
    tail = a.tail.clone() if a.tail is not None else None
    # sequence 0: negative; sequence 1: 200 + 33 overruns cap = 224; sequence 2 is written
    append_tokens_at(a, K, V, [-1, 200, 100], 33)
    want = padded_cache(dev, variant, d, heads, K, V, [0, 0, 133])
    assert torch.equal(a.mem, want.mem), "pos = [-1, 200, 100]"
    # every sequence invalid: nothing is written, the tail included
    before = a.mem.clone()
    tail = a.tail.clone()
    append_tokens_at(a, K, V, [-5, 192, 224], 33)
    torch.cuda.synchronize()
    assert torch.equal(a.mem, before) and torch.equal(a.tail, tail)


# ---- 2. attend (5.: on grouped caches too), 4. invalid lens -----------------------------------------------------------
@pytest.mark.parametrize("heads", HEADS, ids=HEAD_IDS)
@pytest.mark.parametrize("variant,d", BUILT)
def test_attend_tokens_is_the_padded_call(dev, variant, d, heads):
    Q = dev_inputs(dev, d, heads)[0]
    cache = filled(dev, variant, d, heads)
    for lens, Nqs in (([33, 95, 224], (1, 5)), ([1, 64, 193], (1, 5)), ([40, 100, 224], (32, 40)), ([0, 100, 300], (5,))):
        for Nq in Nqs:  # Nq = 32 at s != 0 spans two query groups; Nq = 40 at L = 224 has one group fewer than the grid
            check_attend(dev, cache, Q[:, :Nq].contiguous(), lens, "filled cache")
    assert cache.len == CAP  # the host length is not touched


# ---- 3. garbage behind the open group, nothing readable behind Q ------------------------------------------------------
@pytest.mark.parametrize("variant,d", BUILT)
def test_rows_behind_the_open_group_are_never_read(dev, variant, d):
    """Rows of magnitude 1e30 (inf in Kh, huge sK / sV) behind ceil32(lens[b]): the clean cache's bits.  Q is a fresh
    allocation of exactly its Nq rows, so the rows a padded block would hold around them do not exist."""
    Q, K, V = dev_inputs(dev, d, HEADS[0])
    clean = filled(dev, variant, d, HEADS[0])
    for lens, Nq in (([33, 95, 193], 1), ([40, 100, 160], 40)):
        dirty_k, dirty_v = K.clone(), V.clone()
        for b, L in enumerate(lens):
            dirty_k[b, ceil32(L):] = 1e30
            dirty_v[b, ceil32(L):] = -1e30
        dirty = filled(dev, variant, d, HEADS[0], dirty_k, dirty_v)
        q = torch.empty((B, Nq, Q.shape[2]), dtype=torch.float32, device=dev)
        q.copy_(Q[:, :Nq])
        got = check_attend(dev, dirty, q, lens, "dirty cache", yard=clean)
        assert np.isfinite(got).all()


# ---- 6. against float64 -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dist", rr.DISTS)
@pytest.mark.parametrize("variant,d", BUILT)
def test_against_float64(dev, variant, d, dist):
    """A cache built by append_tokens alone, attended at ragged lengths, at the bounds of tests/test_tokens_cpu.py: int8
    within 5e-3, fp16 within max(1e-3, 1e-3 |ref|) of float64 attention over the real rows.  Every row sees at least
    33 keys, as there."""
    h = HEADS[0][0]
    Qh, Kh, Vh = host_inputs(d, HEADS[0], dist)
    Q, K, V = dev_inputs(dev, d, HEADS[0], dist)
    for lens, Nq in (([95, 193, 224], 5), ([33, 224, 100], 1), ([100, 224, 72], 40)):
        cache = new_cache(dev, variant, d)
        for b, L in enumerate(lens):  # sequence b's L rows in one call, the others left out
            append_tokens_at(cache, K, V, [0 if i == b else -1 for i in range(B)], L)
        got = attend_tokens(cache, Q[:, :Nq].contiguous(), i32(dev, lens))
        for b, L in enumerate(lens):
            ref = rr.attention_f64(Qh[b, :Nq], Kh[b, :L], Vh[b, :L], h * d, h, causal=True)
            err = np.abs(got[b] - ref)
            print(f"{variant} d{d} {dist} L{L} Nq{Nq}: max|gpu - float64| = {float(err.max()):.2e}")
            assert np.isfinite(got[b]).all()
            if variant == INT8:
                assert float(err.max()) <= 5e-3, (lens, Nq, b, float(err.max()))
            else:
                assert (err <= np.maximum(1e-3, 1e-3 * np.abs(ref))).all(), (lens, Nq, b, float(err.max()))


# ---- 7. a decode loop under graph replay --------------------------------------------------------------------------------
@pytest.mark.parametrize("variant,d", [(INT8, 64), (F16, 128)])
def test_decode_loop_under_graph_replay(dev, variant, d):
    """One append_tokens(n = 1) and one attend_tokens(Nq = 1) captured once on a side stream (single stream, linear) over
    static tensors; 35 replays, between which the new K, V, Q rows are copied in and pos / lens advance by 1 on that
    stream.  Sequences 0 and 1 start at 30 and 97 rows (both cross a group boundary); sequence 2 is an empty slot."""
    Q, K, V = dev_inputs(dev, d, HEADS[0])
    start, steps = [30, 97], 35
    cache = new_cache(dev, variant, d)
    cache.mem.copy_(pattern_of(cache))
    for b, L in enumerate(start):
        append_tokens_at(cache, K, V, [0 if i == b else -1 for i in range(B)], L)
    qrow = lambda k: torch.stack([Q[b, k % NQ:k % NQ + 1] for b in range(B)]).contiguous()  # noqa: E731
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    got = []
    with torch.cuda.stream(side):
        qs = torch.zeros((B, 1, Q.shape[2]), dtype=torch.float32, device=dev)
        ks, vs = (torch.zeros((B, 1, K.shape[2]), dtype=torch.float32, device=dev) for _ in range(2))
        buf = torch.full((qs.numel() + 32 * qs.shape[-1],), GUARD, dtype=torch.float32, device=dev)
        pos, lens = i32(dev, [-1] * B), i32(dev, [0] * B)
        cache.append_tokens(ks, vs, pos)  # both kernels once before the capture; every sequence invalid: nothing is placed
        cache.attend_tokens(qs, lens, out=buf[:qs.numel()])
        pos.copy_(i32(dev, start + [-1]))
        lens.copy_(i32(dev, [L + 1 for L in start] + [0]))
        inc = i32(dev, [1, 1, 0])
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            cache.append_tokens(ks, vs, pos)
            cache.attend_tokens(qs, lens, out=buf[:qs.numel()])
        for k in range(steps):
            rows = [L + k for L in start] + [0]
            qs.copy_(qrow(k)), ks.copy_(rows_at(K, rows, 1)), vs.copy_(rows_at(V, rows, 1))
            graph.replay()
            got.append(buf.clone())
            pos.add_(inc), lens.add_(inc)
        side.synchronize()
    torch.cuda.current_stream(dev).wait_stream(side)
    assert pos.tolist() == [30 + steps, 97 + steps, -1] and cache.len == 0
    for k, g in enumerate(got):
        Ls = [L + k + 1 for L in start]
        yard = padded_cache(dev, variant, d, HEADS[0], K, V, Ls + [0])
        g = g.cpu().numpy()
        assert (g[qs.numel():] == GUARD).all(), "O written past its last row"
        o = g[:qs.numel()].reshape(qs.shape)
        for b, L in enumerate(Ls):
            assert_bits(f"replay {k} sequence {b}", o[b], padded_attend(dev, yard, qrow(k), b, L))
        assert_zeros(f"replay {k}: the empty slot", o[2])
    want = padded_cache(dev, variant, d, HEADS[0], K, V, [L + steps for L in start] + [0])
    assert torch.equal(cache.mem, want.mem), "the cache after the loop"


# ---- 8. both bindings -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("heads", [HEADS[0], HEADS[1]], ids=HEAD_IDS[:2])
@pytest.mark.parametrize("variant,d", [(INT8, 64), (F16, 64)])
def test_compiled_binding_gives_the_same_bytes(dev, variant, d, heads):
    Q, K, V = dev_inputs(dev, d, heads)
    q = Q[:, :5].contiguous()
    lens = i32(dev, [45, 71, 0])
    caches = [new_cache(dev, variant, d, heads), new_cache(dev, variant, d, heads, mod=compiled_module())]
    outs = []
    for c in caches:
        c.enable_tokens()  # a second call is a no-op
        append_tokens_at(c, K, V, [0, 0, -1], 38)
        append_tokens_at(c, K, V, [38, 38, -1], 7)
        append_tokens_at(c, K, V, [-1, 45, -1], 26)
        g = Guarded(q)
        c.attend_tokens(q, lens, out=g.buf[:g.n])
        outs.append(g.result())
        plain = c.attend_tokens(q, lens)  # without out: a tensor shaped like Q
        torch.cuda.synchronize()
        assert plain.shape == q.shape and np.array_equal(plain.cpu().numpy(), outs[-1])
    assert torch.equal(caches[0].mem, caches[1].mem)
    if variant == INT8:
        assert torch.equal(caches[0].tail, caches[1].tail)
    assert_bits("compiled against ctypes", outs[1], outs[0])
    assert_zeros("the empty slot", outs[0][2])
    assert np.abs(outs[0][:2]).max() > 0.0
    for mod in (None, compiled_module()):  # dtype, shape and device are checked before the call; int8 needs its tail
        c = new_cache(dev, variant, d, heads, mod=mod, tokens=False)
        if variant == INT8:
            with pytest.raises(RuntimeError, match="needs its tail"):
                c.append_tokens(K[:, :1].contiguous(), V[:, :1].contiguous(), i32(dev, [0] * B))
        with pytest.raises(RuntimeError, match="int32"):
            c.attend_tokens(q, lens.to(torch.int64))
        with pytest.raises(RuntimeError, match="shape"):
            c.attend_tokens(q, lens[:2])
        with pytest.raises(RuntimeError, match="CUDA"):
            c.append_tokens(K[:, :1].contiguous(), V[:, :1].contiguous(), lens.cpu())
