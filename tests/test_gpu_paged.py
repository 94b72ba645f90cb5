"""GPU tests (MI355X) of the paged K/V cache: qmha_kv_cache_append_paged and qmha_attend_cached_paged
through torch_ext.PagedKVCache (ctypes) and the compiled module's class.

A paged call is DEFINED as the token-granular call on a contiguous cache with the row looked up through the block table,
so the yardstick is a contiguous KVCache / GroupedKVCache of cap = 256 fed the same rows through append_tokens, and
every comparison is bit for bit:
  * after append_paged, every page a table names holds, in every array, the contiguous cache's bytes of that sequence
    at rows [pg page_rows, (pg + 1) page_rows); every page no table names keeps the byte pattern both started from (it
    has period 4, so a slice's pattern does not depend on where the slice lies); the tails are equal;
  * attend_paged(Q, lens, table) equals attend_tokens(Q, lens) on the contiguous cache.
Every O is written into the head of a buffer with a sentinel-filled guard behind it.
Shapes: B = 3, h = 2 (grouped: h = 4 on h_kv = 2 or 1), 16 pages of 64 rows (max_pages 4: every stage changes page) or of
128 rows (max_pages 2: every second one does), scrambled tables, every built (variant, d).
"""
import functools
import types

import numpy as np
import pytest

from tests import gpu_support as gs
from tests import rect_ref as rr
from tests.gpu_support import BUILT, F16, GUARD, INT8, Guarded, assert_bits, assert_zeros, compiled_module, dev, i32, to_dev  # noqa: F401

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
B, CAP, NQ, NUM_PAGES = 3, 256, 64, 16
HEADS = [(2, None), (4, 2), (4, 1)]  # (h, h_kv); None: multi-head
HEAD_IDS = ["mha", "gqa2", "gqa1"]
PAGES = [64, 128]  # page_rows; max_pages = CAP / page_rows
# scrambled, non-monotonic, no page named twice
TABLES = {64: [[11, 2, 7, 0], [5, 14, 9, 3], [8, 1, 13, 6]], 128: [[11, 2], [5, 14], [8, 1]]}


def table_for(page_rows, rows=None):
    """The table of `page_rows`, with -1 behind the pages that rows[b] rows of sequence b use (None: all of them)."""
    t = [list(r) for r in TABLES[page_rows]]
    if rows is not None:
        for b, L in enumerate(rows):
            for c in range(-(-L // page_rows), len(t[b])):
                t[b][c] = -1
    return t


def table_dev(dev, table):
    return torch.tensor(table, dtype=torch.int32, device=dev)


@functools.lru_cache(maxsize=None)
def host_inputs(d, heads):
    """Q [B, NQ, h d], K, V [B, CAP, h_kv d]."""
    h, h_kv = heads
    seed = 9900 + d + 10 * h + (h_kv or 0)
    Q = rr.inputs(NQ, CAP, h * d, B, "normal", seed)[0]
    _, K, V = rr.inputs(NQ, CAP, (h_kv or h) * d, B, "normal", seed + 1)
    return Q, K, V


_DEV = {}


def dev_inputs(dev, d, heads):
    key = (d, heads)
    if key not in _DEV:
        _DEV[key] = to_dev(dev, *host_inputs(d, heads))
    return _DEV[key]


def pattern_like(mem):
    """Period 4: every array of a carve starts on a multiple of 256 and every slice, page and group on a multiple of 4."""
    return torch.tensor([0x5A, 0xC3, 0x3C, 0xA5], dtype=torch.uint8, device=mem.device).repeat(-(-mem.numel() // 4))[:mem.numel()].clone()


def new_pool(dev, variant, d, heads, page_rows, mod=None, tokens=True, pattern=True):
    if mod is None:
        from quantizedmha_amd import torch_ext as mod
    h, h_kv = heads
    c = mod.PagedKVCache(B, NUM_PAGES, page_rows, CAP // page_rows, h * d, h, h_kv, variant, str(dev))
    if tokens:
        c.enable_tokens()
    if pattern:
        c.mem.copy_(pattern_like(c.mem))
    return c


def new_yard(dev, variant, d, heads, pattern=True):
    c = gs.new_cache(dev, variant, B, CAP, d, *heads)
    c.enable_tokens()
    if pattern:
        c.mem.copy_(pattern_like(c.mem))
    return c


def pool_arrays(mem, variant, d, heads, page_rows):
    """{array: [NUM_PAGES, h_kv, bytes of a page slice]} over the pool's memory: the carve at B := NUM_PAGES, N := page_rows."""
    h, h_kv = heads
    shim = types.SimpleNamespace(B=NUM_PAGES, num_kv_heads=h_kv or h, cap=page_rows, d_model=h * d, num_heads=h, kernel=variant, mem=mem)
    return {name: gs.cache_array(shim, name, torch.uint8).view(NUM_PAGES, h_kv or h, -1) for name in gs.cache_layout(shim)}


def assert_pool(pool, yard, table, variant, d, heads, page_rows, label):
    """Every page `table` names (entries >= 0) against the contiguous cache's rows; every other page against the pattern."""
    h, h_kv = heads
    hk = h_kv or h
    t = torch.tensor(table, dtype=torch.int64, device=pool.mem.device)
    named = t >= 0
    got = pool_arrays(pool.mem, variant, d, heads, page_rows)
    clean = pool_arrays(pattern_like(pool.mem), variant, d, heads, page_rows)
    free = torch.ones(NUM_PAGES, dtype=torch.bool, device=pool.mem.device)
    free[t[named]] = False
    assert int(free.sum()) == NUM_PAGES - int(named.sum()), "a page is named twice"
    for name, pa in got.items():
        ya = gs.cache_array(yard, name, torch.uint8).view(B, hk, t.shape[1], -1).permute(0, 2, 1, 3)  # [B, max_pages, h_kv, bytes]
        assert ya.shape[3] == pa.shape[2], (name, ya.shape, pa.shape)
        assert torch.equal(pa[t.clamp(min=0)][named], ya[named]), f"{label}: {name} of the named pages"
        assert torch.equal(pa[free], clean[name][free]), f"{label}: {name} of a page no table names was written"
    if variant == INT8:
        assert torch.equal(pool.tail, yard.tail), f"{label}: the tail"


def rows_at(X, pos, n):
    """[B, n, w]: sequence b's rows [pos[b], pos[b] + n) of X (rows [0, n) where pos[b] is invalid)."""
    return torch.stack([X[b, p:p + n] if 0 <= p <= CAP - n else X[b, :n] for b, p in enumerate(pos)]).contiguous()


def append_both(pool, yard, K, V, pos, n, table):
    """Rows [pos[b], pos[b] + n) of K, V into both caches."""
    k, v, p = rows_at(K, pos, n), rows_at(V, pos, n), i32(K.device, pos)
    pool.append_paged(k, v, p, table_dev(K.device, table))
    yard.append_tokens(k, v, p)


def attend_paged(pool, Q, lens, table):
    g = Guarded(Q)
    pool.attend_paged(Q, i32(Q.device, lens), table_dev(Q.device, table), out=g.buf[:g.n])
    return g.result()


def attend_tokens(yard, Q, lens):
    g = Guarded(Q)
    yard.attend_tokens(Q, i32(Q.device, lens), out=g.buf[:g.n])
    return g.result()


def filled(dev, variant, d, heads, page_rows, K=None, V=None):
    """A pool and a contiguous cache whose CAP rows per sequence are all written, in one call."""
    _, K0, V0 = dev_inputs(dev, d, heads)
    pool, yard = new_pool(dev, variant, d, heads, page_rows), new_yard(dev, variant, d, heads)
    append_both(pool, yard, K0 if K is None else K, V0 if V is None else V, [0] * B, CAP, table_for(page_rows))
    return pool, yard


def check_attend(pool, yard, Q, lens, table, label):
    """attend_paged against attend_tokens, per sequence; a length outside [Nq, CAP] gives positive zeros."""
    got, want = attend_paged(pool, Q, lens, table), attend_tokens(yard, Q, lens)
    for b, L in enumerate(lens):
        what = f"{label} lens {lens} Nq {Q.shape[1]} sequence {b}"
        if Q.shape[1] <= L <= CAP:
            assert_bits(what, got[b], want[b])
            assert np.abs(got[b]).max() > 0.0, what
        else:
            assert_zeros(what + " (invalid)", got[b])
    return got


# ---- 1. append (6.: on grouped caches too) ------------------------------------------------------------------------------
@pytest.mark.parametrize("page_rows", PAGES)
@pytest.mark.parametrize("heads", [HEADS[0], HEADS[1]], ids=HEAD_IDS[:2])
@pytest.mark.parametrize("variant,d", BUILT)
def test_append_paged_writes_the_contiguous_bytes(dev, variant, d, heads, page_rows):
    _, K, V = dev_inputs(dev, d, heads)
    pos = [0, 31, 64]
    for n in (1, 7, 33, 70):
        pool, yard = new_pool(dev, variant, d, heads, page_rows), new_yard(dev, variant, d, heads)
        table = table_for(page_rows, [p + n for p in pos])  # -1 behind each sequence's used pages
        # what lies ahead of pos[b]: 31 rows of sequence 1 built token-wise from row 0 (they fill the tail), 64 of sequence 2
        append_both(pool, yard, K, V, [-1, 0, -1], 31, table)
        append_both(pool, yard, K, V, [-1, -1, 0], 64, table)
        append_both(pool, yard, K, V, pos, n, table)
        torch.cuda.synchronize()
        assert not torch.equal(pool.mem, pattern_like(pool.mem))
        assert_pool(pool, yard, table, variant, d, heads, page_rows, f"n = {n} at pos = {pos}")
    # 70 rows at row 60 cross a page boundary inside one call (two of them at 64 rows a page)
    pool, yard = new_pool(dev, variant, d, heads, page_rows), new_yard(dev, variant, d, heads)
    table = table_for(page_rows, [130, 0, 130])
    append_both(pool, yard, K, V, [0, -1, 0], 60, table)
    append_both(pool, yard, K, V, [60, -1, 60], 70, table)
    assert_pool(pool, yard, table, variant, d, heads, page_rows, "n = 70 at pos = 60")


@pytest.mark.parametrize("variant,d", BUILT)
def test_single_token_appends_cross_page_boundaries(dev, variant, d):
    """30 rows, then one row at a time up to 70 (sequence 2: 96 rows further on): after every call every named page is the
    contiguous cache's.  64 rows a page: sequences 0 and 1 enter their second page, sequence 2 its third."""
    _, K, V = dev_inputs(dev, d, HEADS[0])
    off = [0, 0, 96]
    pool, yard = new_pool(dev, variant, d, HEADS[0], 64), new_yard(dev, variant, d, HEADS[0])
    append_both(pool, yard, K, V, [-1, -1, 0], 96, table_for(64, [0, 0, 96]))
    append_both(pool, yard, K, V, off, 30, table_for(64, [30, 30, 126]))
    for L in range(30, 70):
        table = table_for(64, [o + L + 1 for o in off])
        append_both(pool, yard, K, V, [o + L for o in off], 1, table)
        assert_pool(pool, yard, table, variant, d, HEADS[0], 64, f"after the row at {L}")


# ---- 2. attend (6.: on grouped caches too), 5. invalid lengths ----------------------------------------------------------
@pytest.mark.parametrize("page_rows", PAGES)
@pytest.mark.parametrize("heads", HEADS, ids=HEAD_IDS)
@pytest.mark.parametrize("variant,d", BUILT)
def test_attend_paged_is_attend_tokens(dev, variant, d, heads, page_rows):
    Q = dev_inputs(dev, d, heads)[0]
    pool, yard = filled(dev, variant, d, heads, page_rows)
    for lens, Nqs in (([33, 95, 224], (1, 5)), ([1, 64, 193], (1, 5)), ([40, 100, 224], (32, 40)), ([256, 128, 65], (1,)),
                      ([0, 100, 300], (5,))):
        table = table_for(page_rows, [L if L <= CAP else 0 for L in lens])  # -1 behind each sequence's used pages
        for Nq in Nqs:
            q = Q[:, :Nq].contiguous()
            got = check_attend(pool, yard, q, lens, table, f"{page_rows} rows a page")
            # an entry of -1 behind the used pages changes nothing: the full table gives the same bits
            assert_bits("full table", attend_paged(pool, q, lens, table_for(page_rows)), got)


# ---- 3. a shared prefix -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("page_rows", PAGES)
@pytest.mark.parametrize("variant,d", BUILT)
def test_two_sequences_share_a_prefix_page(dev, variant, d, page_rows):
    """Sequences 0 and 1 name the same first page, written once through sequence 0 (sequence 1 left out: pos = -1); each
    then appends its own continuation at pos = page_rows into a page of its own."""
    Q, K, V = dev_inputs(dev, d, HEADS[0])
    n = 37
    Kc, Vc = K.clone(), V.clone()
    Kc[1, :page_rows], Vc[1, :page_rows] = K[0, :page_rows], V[0, :page_rows]  # the contiguous caches hold the prefix twice
    table = table_for(page_rows, [page_rows + n] * B)
    table[1][0] = table[0][0]
    pool, yard = new_pool(dev, variant, d, HEADS[0], page_rows), new_yard(dev, variant, d, HEADS[0])
    k, v = rows_at(Kc, [0] * B, page_rows), rows_at(Vc, [0] * B, page_rows)
    pool.append_paged(k, v, i32(dev, [0, -1, 0]), table_dev(dev, table))
    yard.append_tokens(k, v, i32(dev, [0, 0, 0]))
    append_both(pool, yard, Kc, Vc, [page_rows] * B, n, table)
    for Nq in (1, 5):
        check_attend(pool, yard, Q[:, :Nq].contiguous(), [page_rows + n] * B, table, "shared prefix")


# ---- 4. garbage everywhere a call must not look --------------------------------------------------------------------------
@pytest.mark.parametrize("page_rows", PAGES)
@pytest.mark.parametrize("variant,d", BUILT)
def test_pages_and_groups_outside_the_used_rows_are_never_read(dev, variant, d, page_rows):
    """Every page outside a sequence's used pages, and every group at and beyond ceil32(L) inside its last page, holds
    rows of magnitude 1e30 (inf in Kh, huge sK / sV): the clean pool's bits.  Q is a fresh allocation of exactly its Nq rows."""
    Q, K, V = dev_inputs(dev, d, HEADS[0])
    mp = CAP // page_rows
    rounds = -(-NUM_PAGES // (B * mp))  # tables that cover all the pages between them
    cover = [[[(mp * (B * r + b) + c) % NUM_PAGES for c in range(mp)] for b in range(B)] for r in range(rounds)]
    for lens, Nq in (([33, 95, 193], 1), ([40, 100, 160], 40)):
        table = table_for(page_rows, lens)
        outs = []
        for dirty in (False, True):
            pool = new_pool(dev, variant, d, HEADS[0], page_rows)
            if dirty:  # all 16 pages
                big_k, big_v = torch.full_like(K, 1e30), torch.full_like(V, -1e30)
                for t in cover:
                    pool.append_paged(big_k, big_v, i32(dev, [0] * B), table_dev(dev, t))
            for b, L in enumerate(lens):  # sequence b's L rows in one call, the others left out
                pos = [0 if i == b else -1 for i in range(B)]
                pool.append_paged(rows_at(K, pos, L), rows_at(V, pos, L), i32(dev, pos), table_dev(dev, table))
            q = torch.empty((B, Nq, Q.shape[2]), dtype=torch.float32, device=dev)
            q.copy_(Q[:, :Nq])
            outs.append(attend_paged(pool, q, lens, table))
        assert np.isfinite(outs[1]).all()
        assert_bits(f"dirty pool lens {lens} Nq {Nq}", outs[1], outs[0])
        assert all(np.abs(outs[0][b]).max() > 0.0 for b in range(B))


# ---- 5. invalid table entries (6.: on grouped caches too) ------------------------------------------------------------------
@pytest.mark.parametrize("page_rows", PAGES)
@pytest.mark.parametrize("heads", [HEADS[0], HEADS[2]], ids=["mha", "gqa1"])
@pytest.mark.parametrize("variant,d", BUILT)
def test_a_used_entry_outside_the_pool(dev, variant, d, heads, page_rows):
    Q, K, V = dev_inputs(dev, d, heads)
    pool, yard = filled(dev, variant, d, heads, page_rows)
    lens = [33, 95, 224] if page_rows == 64 else [33, 200, 224]  # sequence 1 uses two pages
    q = Q[:, :5].contiguous()
    want = attend_tokens(yard, q, lens)
    for bad in (-1, NUM_PAGES, NUM_PAGES + 1000, -2 ** 31):
        for col in (0, 1):
            table = table_for(page_rows, lens)
            table[1][col] = bad
            got = attend_paged(pool, q, lens, table)
            assert_zeros(f"entry {bad} in column {col}: sequence 1", got[1])
            assert_bits(f"entry {bad} in column {col}: the others", got[[0, 2]], want[[0, 2]])
    # the same entries in an append: nothing of that sequence is written, the tail included; the others are
    for bad in (-1, NUM_PAGES):
        pool, yard = new_pool(dev, variant, d, heads, page_rows), new_yard(dev, variant, d, heads)
        table = table_for(page_rows, [130, 130, 130])
        append_both(pool, yard, K, V, [0, 0, 0], 60, table)
        broken = [list(r) for r in table]
        broken[1][130 // page_rows] = bad  # the page the call's last rows fall into
        k, v = rows_at(K, [60] * B, 70), rows_at(V, [60] * B, 70)
        pool.append_paged(k, v, i32(dev, [60] * B), table_dev(dev, broken))
        yard.append_tokens(k, v, i32(dev, [60, -1, 60]))
        assert_pool(pool, yard, table, variant, d, heads, page_rows, f"append with entry {bad}")
    # pos out of range: beyond the logical capacity, negative
    before, tail = pool.mem.clone(), pool.tail.clone()
    pool.append_paged(k, v, i32(dev, [CAP - 69, -1, CAP]), table_dev(dev, table_for(page_rows)))
    torch.cuda.synchronize()
    assert torch.equal(pool.mem, before) and torch.equal(pool.tail, tail)


# ---- 7. a decode loop under graph replay ----------------------------------------------------------------------------------
@pytest.mark.parametrize("variant,d", [(INT8, 64), (F16, 128)])
def test_decode_loop_under_graph_replay(dev, variant, d):
    """One append_paged(n = 1) and one attend_paged(Nq = 1) captured once on a side stream (single stream, linear) over
    static tensors; 35 replays, between which the new K, V, Q rows are copied in and pos / lens advance by 1 on that
    stream.  Sequences 0 and 1 start at 30 and 97 rows and cross a page boundary (64 rows a page); the entry of the page
    a sequence enters is written on that stream before the replay that needs it.  Sequence 2 is an empty slot."""
    page_rows = 64
    Q, K, V = dev_inputs(dev, d, HEADS[0])
    start, steps = [30, 97], 35
    pool, yard = new_pool(dev, variant, d, HEADS[0], page_rows), new_yard(dev, variant, d, HEADS[0])
    full = table_for(page_rows)
    first = table_for(page_rows, start + [0])
    for b, L in enumerate(start):
        append_both(pool, yard, K, V, [0 if i == b else -1 for i in range(B)], L, first)
    qrow = lambda k: torch.stack([Q[b, k % NQ:k % NQ + 1] for b in range(B)]).contiguous()  # noqa: E731
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    got = []
    with torch.cuda.stream(side):
        qs = torch.zeros((B, 1, Q.shape[2]), dtype=torch.float32, device=dev)
        ks, vs = (torch.zeros((B, 1, K.shape[2]), dtype=torch.float32, device=dev) for _ in range(2))
        buf = torch.full((qs.numel() + 32 * qs.shape[-1],), GUARD, dtype=torch.float32, device=dev)
        pos, lens = i32(dev, [-1] * B), i32(dev, [0] * B)
        table = table_dev(dev, first)
        pool.append_paged(ks, vs, pos, table)  # both kernels once before the capture; every sequence invalid: nothing is placed
        pool.attend_paged(qs, lens, table, out=buf[:qs.numel()])
        pos.copy_(i32(dev, start + [-1]))
        lens.copy_(i32(dev, [L + 1 for L in start] + [0]))
        inc = i32(dev, [1, 1, 0])
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            pool.append_paged(ks, vs, pos, table)
            pool.attend_paged(qs, lens, table, out=buf[:qs.numel()])
        entered = 0
        for k in range(steps):
            rows = [L + k for L in start] + [0]
            for b, r in enumerate(rows[:2]):
                if r % page_rows == 0:  # the row opens a page: name it before the replay that writes there
                    table[b, r // page_rows] = full[b][r // page_rows]
                    entered += 1
            qs.copy_(qrow(k)), ks.copy_(rows_at(K, rows, 1)), vs.copy_(rows_at(V, rows, 1))
            graph.replay()
            got.append(buf.clone())
            pos.add_(inc), lens.add_(inc)
        side.synchronize()
    torch.cuda.current_stream(dev).wait_stream(side)
    assert entered == 2 and pos.tolist() == [30 + steps, 97 + steps, -1]
    for k, g in enumerate(got):  # the eager contiguous path, step by step
        rows = [L + k for L in start] + [-1]
        yard.append_tokens(rows_at(K, rows, 1), rows_at(V, rows, 1), i32(dev, rows))
        want = attend_tokens(yard, qrow(k), [L + k + 1 for L in start] + [0])
        g = g.cpu().numpy()
        assert (g[qs.numel():] == GUARD).all(), "O written past its last row"
        o = g[:qs.numel()].reshape(qs.shape)
        assert_bits(f"replay {k}", o[:2], want[:2])
        assert np.abs(o[:2]).max() > 0.0
        assert_zeros(f"replay {k}: the empty slot", o[2])
    final = table_for(page_rows, [L + steps for L in start] + [0])
    assert table.tolist() == final
    assert_pool(pool, yard, final, variant, d, HEADS[0], page_rows, "the pool after the loop")


# ---- 8. both bindings ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("heads", [HEADS[0], HEADS[1]], ids=HEAD_IDS[:2])
@pytest.mark.parametrize("variant,d", [(INT8, 64), (F16, 64)])
def test_compiled_binding_gives_the_same_bytes(dev, variant, d, heads):
    Q, K, V = dev_inputs(dev, d, heads)
    q = Q[:, :5].contiguous()
    lens = i32(dev, [45, 71, 0])
    table = table_dev(dev, table_for(64, [45, 71, 0]))
    pools = [new_pool(dev, variant, d, heads, 64), new_pool(dev, variant, d, heads, 64, mod=compiled_module())]
    outs = []
    for c in pools:
        c.enable_tokens()  # a second call is a no-op
        for pos, n in (([0, 0, -1], 38), ([38, 38, -1], 7), ([-1, 45, -1], 26)):
            c.append_paged(rows_at(K, pos, n), rows_at(V, pos, n), i32(dev, pos), table)
        g = Guarded(q)
        c.attend_paged(q, lens, table, out=g.buf[:g.n])
        outs.append(g.result())
        plain = c.attend_paged(q, lens, table)  # without out: a tensor shaped like Q
        torch.cuda.synchronize()
        assert plain.shape == q.shape and np.array_equal(plain.cpu().numpy(), outs[-1])
        assert c.cap == CAP
    assert torch.equal(pools[0].mem, pools[1].mem) and not torch.equal(pools[0].mem, pattern_like(pools[0].mem))
    if variant == INT8:
        assert torch.equal(pools[0].tail, pools[1].tail)
    assert_bits("compiled against ctypes", outs[1], outs[0])
    assert_zeros("the empty slot", outs[0][2])
    assert np.abs(outs[0][:2]).max() > 0.0
    k1, v1 = K[:, :1].contiguous(), V[:, :1].contiguous()
    for mod in (None, compiled_module()):  # dtype, shape and device are checked before the call; int8 needs its tail
        c = new_pool(dev, variant, d, heads, 64, mod=mod, tokens=False)
        if variant == INT8:
            with pytest.raises(RuntimeError, match="needs its tail"):
                c.append_paged(k1, v1, i32(dev, [0] * B), table)
        with pytest.raises(RuntimeError, match="int32"):
            c.attend_paged(q, lens, table.to(torch.int64))
        with pytest.raises(RuntimeError, match="int32"):
            c.attend_paged(q, lens.to(torch.int64), table)
        with pytest.raises(RuntimeError, match="shape"):
            c.attend_paged(q, lens, table[:, :3])
        with pytest.raises(RuntimeError, match="shape"):
            c.attend_paged(q, lens, table.t().contiguous().t())  # [B, max_pages], not contiguous
        with pytest.raises(RuntimeError, match="shape"):
            c.append_paged(k1, v1, lens[:2], table)
        with pytest.raises(RuntimeError, match="CUDA"):
            c.append_paged(k1, v1, lens, table.cpu())
        with pytest.raises(RuntimeError, match="page_rows"):
            type(c)(B, NUM_PAGES, 96, 4, heads[0] * d, heads[0], heads[1], variant, str(dev))
