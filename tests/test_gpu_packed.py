"""GPU tests (MI355X) of the packed-batch calls: append_packed / attend_packed of KVCache and
GroupedKVCache, append_paged_packed / attend_paged_packed of PagedKVCache, through the ctypes binding and the compiled
module.

A packed call is DEFINED by what shipped before it: a sequence with n_b rows gets, bit for bit, what append_tokens /
attend_tokens (or the paged calls) give a batch of that row count.  The yardstick builders of tests/packed_ref.py run
those calls once per distinct count on a padded [B, c, ...] buffer with the other sequences switched off, and every
comparison here is bit for bit against them.  Every O is the head of a buffer filled with a sentinel and followed by a
guard: rows outside every range, and rows of a sequence whose range is out of bounds, must keep the sentinel.
Shapes: B = 4, cap = 224 (a partial last stage), h = 2 (grouped: h = 4 on h_kv = 2 or 1), every built (variant, d); pools of
20 pages of 64 or 128 rows (256 logical rows) under permuted tables.
"""
import functools
import types

import numpy as np
import pytest

from tests import gpu_support as gs
from tests import packed_ref as pk
from tests import rect_ref as rr
from tests.gpu_support import BUILT, F16, GUARD, INT8, Guarded, assert_bits, assert_zeros, compiled_module, dev, i32, to_dev  # noqa: F401

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
B, CAP, PCAP, NQ, NUM_PAGES = 4, 224, 256, 64, 20
HEADS = [(2, None), (4, 2), (4, 1)]  # (h, h_kv); None: multi-head
HEAD_IDS = ["mha", "gqa2", "gqa1"]
PAGES = [64, 128]  # page_rows; max_pages = PCAP / page_rows
# permuted, non-monotonic, no page named twice; pages 12, 15, 16, 18 (64) are named by no table
TABLES = {64: [[11, 2, 7, 0], [5, 14, 9, 3], [8, 1, 13, 6], [17, 4, 19, 10]], 128: [[11, 2], [5, 14], [8, 1], [17, 4]]}
SPARE = 3.5  # what the rows of a packed operand outside every range hold


@functools.lru_cache(maxsize=None)
def host_inputs(d, heads):
    """Q [B, NQ, h d], K, V [B, PCAP, h_kv d]."""
    h, h_kv = heads
    seed = 7700 + d + 10 * h + (h_kv or 0)
    Q = rr.inputs(NQ, PCAP, h * d, B, "normal", seed)[0]
    _, K, V = rr.inputs(NQ, PCAP, (h_kv or h) * d, B, "normal", seed + 1)
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


def new_cache(dev, variant, d, heads, cap=CAP, mod=None, tokens=True):
    c = gs.new_cache(dev, variant, B, cap, d, *heads, mod=mod)
    if tokens:
        c.enable_tokens()
    c.mem.copy_(pattern_like(c.mem))
    return c


def new_pool(dev, variant, d, heads, page_rows, mod=None, tokens=True):
    if mod is None:
        from quantizedmha_amd import torch_ext as mod
    h, h_kv = heads
    c = mod.PagedKVCache(B, NUM_PAGES, page_rows, PCAP // page_rows, h * d, h, h_kv, variant, str(dev))
    if tokens:
        c.enable_tokens()
    c.mem.copy_(pattern_like(c.mem))
    return c


def table_dev(dev, table):
    return torch.tensor(table, dtype=torch.int32, device=dev)


def cu_of(counts):
    return [int(x) for x in np.concatenate([[0], np.cumsum(counts)])]


def packed(X, cu, total, starts=None):
    """[total, w]: rows [cu[b], cu[b + 1]) hold X[b, starts[b] : starts[b] + count_b] (starts: 0), every other row SPARE.  A
    fresh allocation of exactly `total` rows."""
    P = torch.empty((total, X.shape[2]), dtype=torch.float32, device=X.device)
    P.fill_(SPARE)
    for b in range(len(cu) - 1):
        s = 0 if starts is None else starts[b]
        P[cu[b]:cu[b + 1]] = X[b, s:s + cu[b + 1] - cu[b]]
    return P


def rows_at(X, pos, n, cap):
    """[B, n, w]: sequence b's rows [pos[b], pos[b] + n) of X (rows [0, n) where pos[b] is invalid)."""
    return torch.stack([X[b, p:p + n] if 0 <= p <= cap - n else X[b, :n] for b, p in enumerate(pos)]).contiguous()


def tokens_append(cache, table=None):
    """append_tokens (append_paged through `table`) as packed_ref.yard_append calls it."""
    if table is None:
        return lambda Kpad, Vpad, pos: cache.append_tokens(Kpad, Vpad, i32(Kpad.device, pos))
    return lambda Kpad, Vpad, pos: cache.append_paged(Kpad, Vpad, i32(Kpad.device, pos), table_dev(Kpad.device, table))


def tokens_attend(cache, table=None):
    """attend_tokens (attend_paged through `table`) as packed_ref.yard_attend calls it: numpy through the guard."""
    def call(Qpad, lens):
        g = Guarded(Qpad)
        if table is None:
            cache.attend_tokens(Qpad, i32(Qpad.device, lens), out=g.buf[:g.n])
        else:
            cache.attend_paged(Qpad, i32(Qpad.device, lens), table_dev(Qpad.device, table), out=g.buf[:g.n])
        return g.result()
    return call


def append_packed(cache, Kp, Vp, cu, pos, max_n, table=None):
    dv = Kp.device
    if table is None:
        cache.append_packed(Kp, Vp, i32(dv, cu), i32(dv, pos), max_n)
    else:
        cache.append_paged_packed(Kp, Vp, i32(dv, cu), i32(dv, pos), table_dev(dv, table), max_n)


def attend_packed(cache, Qp, cu, lens, max_nq, table=None):
    """O [total, d_model] (numpy) through the guard; it starts as the sentinel."""
    dv, g = Qp.device, Guarded(Qp)
    if table is None:
        cache.attend_packed(Qp, i32(dv, cu), i32(dv, lens), max_nq, out=g.out)
    else:
        cache.attend_paged_packed(Qp, i32(dv, cu), i32(dv, lens), table_dev(dv, table), max_nq, out=g.out)
    return g.result()


def assert_packed(label, got, cu, want, zeros=()):
    """Rows [cu[b], cu[b + 1]) of `got`: want[b] bit for bit; positive zeros for b in `zeros`; every other row the sentinel."""
    exp = np.full_like(got, GUARD)
    for b, rows in want.items():
        exp[cu[b]:cu[b + 1]] = rows
        assert np.abs(rows).max() > 0.0, (label, b)
    for b in zeros:
        assert_zeros(f"{label}: sequence {b} (invalid)", got[cu[b]:cu[b + 1]])
        exp[cu[b]:cu[b + 1]] = 0.0
    assert_bits(label, got, exp)


def filled(dev, variant, d, heads, K=None, V=None):
    """A cache whose CAP rows per sequence are all written, in one append_tokens."""
    _, K0, V0 = dev_inputs(dev, d, heads)
    c = new_cache(dev, variant, d, heads)
    K, V = K0 if K is None else K, V0 if V is None else V
    c.append_tokens(K[:, :CAP].contiguous(), V[:, :CAP].contiguous(), i32(dev, [0] * B))
    return c


def assert_same_cache(label, a, b, variant):
    torch.cuda.synchronize()
    assert torch.equal(a.mem, b.mem), f"{label}: the cache bytes"
    assert not torch.equal(a.mem, pattern_like(a.mem)), f"{label}: nothing was written"
    if variant == INT8:
        assert torch.equal(a.tail, b.tail), f"{label}: the tail"


# the mixes of the attend tests: (counts, lens, total, max_nq).  The first has four spare rows and an empty sequence; in the
# second a count of 32 at s != 0 spans two query groups, and 5 beside 40 has fewer active groups than the grid
MIXES = [([1, 5, 0, 40], [33, 95, 7, 224], 50, 40), ([32, 1, 40, 5], [40, 1, 224, 100], 80, 40)]


# ---- 1. attend ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("heads", HEADS, ids=HEAD_IDS)
@pytest.mark.parametrize("variant,d", BUILT)
def test_attend_packed_is_attend_tokens_per_sequence(dev, variant, d, heads):
    Q = dev_inputs(dev, d, heads)[0]
    cache = filled(dev, variant, d, heads)
    for counts, lens, total, max_nq in MIXES:
        cu = cu_of(counts)
        assert cu[-1] < total  # spare rows behind the last range
        Qp = packed(Q, cu, total)
        want = pk.yard_attend(tokens_attend(cache), Qp, cu, lens)
        assert sorted(want) == [b for b in range(B) if counts[b]]
        got = attend_packed(cache, Qp, cu, lens, max_nq)
        assert_packed(f"counts {counts} lens {lens}", got, cu, want)
        # a larger bound sizes a larger grid and gives the same bits
        if max_nq < total:
            assert_bits("max_nq = total", attend_packed(cache, Qp, cu, lens, min(total, CAP)), got)


# ---- 2. append ------------------------------------------------------------------------------------------------------------
def append_setup(dev, variant, d, heads, cap=CAP, page_rows=None):
    """The cache under test and the yardstick's, both over one byte pattern, holding sequence 0's first 31 rows (built
    token-wise from row 0: they fill the tail) and sequence 3's first 64."""
    _, K, V = dev_inputs(dev, d, heads)
    table = None if page_rows is None else TABLES[page_rows]
    pc = new_cache(dev, variant, d, heads, cap) if page_rows is None else new_pool(dev, variant, d, heads, page_rows)
    yc = new_cache(dev, variant, d, heads, cap)
    for pos, n in (([0, -1, -1, -1], 31), ([-1, -1, -1, 0], 64)):
        k, v = rows_at(K, pos, n, cap), rows_at(V, pos, n, cap)
        tokens_append(pc, table)(k, v, pos)
        tokens_append(yc)(k, v, pos)
    return pc, yc, table


APPEND_1 = ([1, 33, 0, 70], [31, 0, 5, 64], 106, 70)  # counts, pos, total (two spare rows), max_n
APPEND_2 = ([7, 40, 3, 30], [32, 33, 0, 134], 80, 40)  # continues every open group


@pytest.mark.parametrize("heads", [HEADS[0], HEADS[1]], ids=HEAD_IDS[:2])
@pytest.mark.parametrize("variant,d", BUILT)
def test_append_packed_writes_append_tokens_bytes(dev, variant, d, heads):
    _, K, V = dev_inputs(dev, d, heads)
    pc, yc, _ = append_setup(dev, variant, d, heads)
    for counts, pos, total, max_n in (APPEND_1, APPEND_2):
        cu = cu_of(counts)
        Kp, Vp = packed(K, cu, total, pos), packed(V, cu, total, pos)
        append_packed(pc, Kp, Vp, cu, pos, max_n)
        pk.yard_append(tokens_append(yc), Kp, Vp, cu, pos)
        # the whole cache tensor and the tail over one byte pattern: nothing outside the touched groups is written
        assert_same_cache(f"counts {counts} at pos {pos}", pc, yc, variant)


# ---- 3. invalid entries, one at a time --------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant,d", BUILT)
def test_attend_packed_invalid_entries(dev, variant, d):
    heads = HEADS[0]
    Q = dev_inputs(dev, d, heads)[0]
    cache = filled(dev, variant, d, heads)
    counts, lens, total, max_nq = MIXES[0]
    cu = cu_of(counts)  # [0, 1, 6, 6, 46]
    Qp = packed(Q, cu, total)
    want = pk.yard_attend(tokens_attend(cache), Qp, cu, lens)
    before, tail = cache.mem.clone(), cache.tail.clone()

    def case(label, cu_call=cu, lens_call=lens, bound=max_nq, skipped=(), zeros=()):
        got = attend_packed(cache, Qp, cu_call, lens_call, bound)
        keep = {b: w for b, w in want.items() if b not in skipped and b not in zeros}
        assert_packed(label, got, cu, keep, zeros)

    case("a decreasing cu pair", cu_call=[0, 1, 6, 6, 4], skipped=[3])  # nothing of that sequence is read or written
    case("cu[b + 1] > total", cu_call=[0, 1, 6, 6, total + 1], skipped=[3])
    case("a negative cu[b]", cu_call=[-1, 1, 6, 6, 46], skipped=[0])
    case("nq_b > max_nq", bound=39, zeros=[3])
    case("L < nq_b", lens_call=[33, 4, 7, 224], zeros=[1])
    case("L > cap", lens_call=[33, 95, 7, CAP + 1], zeros=[3])
    case("a negative L", lens_call=[-1, 95, 7, 224], zeros=[0])
    # every sequence invalid: the zeroed ranges apart, O keeps its bytes; the cache and the tail keep theirs
    case("every sequence invalid", lens_call=[0, 4, 7, 300], zeros=[0, 1, 3])
    torch.cuda.synchronize()
    assert torch.equal(cache.mem, before) and torch.equal(cache.tail, tail)


@pytest.mark.parametrize("variant,d", BUILT)
def test_append_packed_invalid_entries(dev, variant, d):
    heads = HEADS[0]
    _, K, V = dev_inputs(dev, d, heads)
    counts, pos, total, max_n = APPEND_1
    cu = cu_of(counts)  # [0, 1, 34, 34, 104]
    Kp, Vp = packed(K, cu, total, pos), packed(V, cu, total, pos)
    for label, cu_call, pos_call, bound, skipped in (
            ("a decreasing cu pair", [0, 1, 34, 34, 30], pos, max_n, [3]),
            ("cu[b + 1] > total", [0, 1, 34, 34, total + 1], pos, max_n, [3]),
            ("a negative cu[b]", [-1, 1, 34, 34, 104], pos, max_n, [0]),
            ("n_b > max_n", cu, pos, 69, [3]),
            ("pos[b] < 0", cu, [31, -1, 5, 64], max_n, [1]),
            ("pos[b] + n_b > cap", cu, [31, 0, 5, CAP - 69], max_n, [3])):
        pc, yc, _ = append_setup(dev, variant, d, heads)
        append_packed(pc, Kp, Vp, cu_call, pos_call, bound)
        pk.yard_append(tokens_append(yc), Kp, Vp, cu, pos, skip=skipped)  # the others keep their bits
        assert_same_cache(label, pc, yc, variant)
    # every sequence invalid (sequence 2 is empty): the cache and the tail keep their bytes
    pc, _, _ = append_setup(dev, variant, d, heads)
    torch.cuda.synchronize()
    before, tail = pc.mem.clone(), pc.tail.clone()
    append_packed(pc, Kp, Vp, cu, [-1, CAP - 32, 5, CAP - 69], max_n)
    append_packed(pc, Kp, Vp, [5, 4, 3, 2, 1], pos, max_n)
    append_packed(pc, Kp, Vp, [0, 0, 0, 0, 0], [-1] * B, max_n)  # every sequence empty
    torch.cuda.synchronize()
    assert torch.equal(pc.mem, before) and torch.equal(pc.tail, tail)


# ---- 4. garbage everywhere a call must not look --------------------------------------------------------------------------
@pytest.mark.parametrize("variant,d", BUILT)
def test_rows_behind_ceil32_of_the_length_are_never_read(dev, variant, d):
    """Rows of magnitude 1e30 in every group at and beyond ceil32(L) (inf in Kh, huge sK / sV): the clean cache's bits.  Q is
    a fresh allocation of exactly `total` rows."""
    heads = HEADS[0]
    Q, K, V = dev_inputs(dev, d, heads)
    for counts, lens, total, max_nq in MIXES:
        cu = cu_of(counts)
        outs = []
        for dirty in (False, True):
            c = new_cache(dev, variant, d, heads)
            if dirty:
                big_k, big_v = torch.full_like(K[:, :CAP], 1e30), torch.full_like(V[:, :CAP], -1e30)
                c.append_tokens(big_k.contiguous(), big_v.contiguous(), i32(dev, [0] * B))
            for b, L in enumerate(lens):  # sequence b's L rows in one call, the others left out
                pos = [0 if i == b else -1 for i in range(B)]
                c.append_tokens(rows_at(K, pos, L, CAP), rows_at(V, pos, L, CAP), i32(dev, pos))
            outs.append(attend_packed(c, packed(Q, cu, total), cu, lens, max_nq))
        assert np.isfinite(outs[1]).all()
        assert_bits(f"dirty cache, counts {counts}", outs[1], outs[0])
        assert all(np.abs(outs[0][cu[b]:cu[b + 1]]).max() > 0.0 for b in range(B) if counts[b])


# ---- 5. paged -------------------------------------------------------------------------------------------------------------
def pool_arrays(mem, variant, d, heads, page_rows):
    """{array: [NUM_PAGES, h_kv, bytes of a page slice]} over the pool's memory: the carve at B := NUM_PAGES, N := page_rows."""
    h, h_kv = heads
    shim = types.SimpleNamespace(B=NUM_PAGES, num_kv_heads=h_kv or h, cap=page_rows, d_model=h * d, num_heads=h, kernel=variant, mem=mem)
    return {name: gs.cache_array(shim, name, torch.uint8).view(NUM_PAGES, h_kv or h, -1) for name in gs.cache_layout(shim)}


def assert_pool(pool, yard, table, variant, d, heads, page_rows, label, shared=()):
    """Every page `table` names against the contiguous cache's rows; every other page against the pattern.  `shared`:
    (b, column) entries that name a page another entry names too."""
    h, h_kv = heads
    hk = h_kv or h
    torch.cuda.synchronize()
    t = torch.tensor(table, dtype=torch.int64, device=pool.mem.device)
    got = pool_arrays(pool.mem, variant, d, heads, page_rows)
    clean = pool_arrays(pattern_like(pool.mem), variant, d, heads, page_rows)
    free = torch.ones(NUM_PAGES, dtype=torch.bool, device=pool.mem.device)
    free[t.flatten()] = False
    assert int(free.sum()) == NUM_PAGES - t.numel() + len(shared), "a page is named twice"
    for name, pa in got.items():
        ya = gs.cache_array(yard, name, torch.uint8).view(B, hk, t.shape[1], -1).permute(0, 2, 1, 3)  # [B, max_pages, h_kv, bytes]
        assert torch.equal(pa[t], ya), f"{label}: {name} of the named pages"
        assert torch.equal(pa[free], clean[name][free]), f"{label}: {name} of a page no table names was written"
    if variant == INT8:
        assert torch.equal(pool.tail, yard.tail), f"{label}: the tail"


@pytest.mark.parametrize("page_rows", PAGES)
@pytest.mark.parametrize("heads", [HEADS[0], HEADS[2]], ids=["mha", "gqa1"])
@pytest.mark.parametrize("variant,d", BUILT)
def test_paged_packed_calls_equal_the_contiguous_ones(dev, variant, d, heads, page_rows):
    Q, K, V = dev_inputs(dev, d, heads)
    pool, cache, table = append_setup(dev, variant, d, heads, PCAP, page_rows)
    yard = append_setup(dev, variant, d, heads, PCAP)[0]  # the token calls' bytes, to hold both packed caches to
    for counts, pos, total, max_n in (APPEND_1, APPEND_2):
        cu = cu_of(counts)
        Kp, Vp = packed(K, cu, total, pos), packed(V, cu, total, pos)
        append_packed(pool, Kp, Vp, cu, pos, max_n, table)
        append_packed(cache, Kp, Vp, cu, pos, max_n)
        pk.yard_append(tokens_append(yard), Kp, Vp, cu, pos)
        assert_pool(pool, cache, table, variant, d, heads, page_rows, f"append counts {counts}")
        assert_same_cache(f"append counts {counts}", cache, yard, variant)
    held = [39, 73, 3, 164]  # rows each sequence holds now
    for counts, total in (([1, 5, 0, 40], 50), ([32, 1, 40, 5], 80), ([39, 40, 3, 1], 85)):
        cu = cu_of(counts)
        Qp = packed(Q, cu, total)
        got = attend_packed(pool, Qp, cu, held, 40, table)
        assert_bits(f"attend counts {counts}", got, attend_packed(cache, Qp, cu, held, 40))
        want = pk.yard_attend(tokens_attend(pool, table), Qp, cu, held, skip=[b for b in range(B) if counts[b] > held[b]])
        assert_packed(f"attend counts {counts} against attend_paged", got, cu, want, zeros=[b for b in range(B) if counts[b] > held[b]])


@pytest.mark.parametrize("page_rows", PAGES)
@pytest.mark.parametrize("variant,d", BUILT)
def test_two_sequences_share_a_prefix_page(dev, variant, d, page_rows):
    """Sequences 0 and 1 name the same first page, written once through sequence 0 (sequence 1 brings no rows); each then
    appends its own continuation at pos = page_rows into a page of its own, and sequence 2 takes no part."""
    heads = HEADS[0]
    Q, K, V = dev_inputs(dev, d, heads)
    n = 37
    Kc, Vc = K.clone(), V.clone()
    Kc[1, :page_rows], Vc[1, :page_rows] = K[0, :page_rows], V[0, :page_rows]  # the contiguous cache holds the prefix twice
    table = [list(r) for r in TABLES[page_rows]]
    table[1][0] = table[0][0]
    pool, cache = new_pool(dev, variant, d, heads, page_rows), new_cache(dev, variant, d, heads, PCAP)
    cu = cu_of([page_rows, 0, 0, 0])
    append_packed(pool, packed(Kc, cu, page_rows), packed(Vc, cu, page_rows), cu, [0] * B, page_rows, table)
    cu2 = cu_of([page_rows, page_rows, 0, 0])
    append_packed(cache, packed(Kc, cu2, 2 * page_rows), packed(Vc, cu2, 2 * page_rows), cu2, [0] * B, page_rows)
    cu3, pos = cu_of([n, n, 0, 5]), [page_rows, page_rows, 0, 0]
    Kp, Vp = packed(Kc, cu3, 2 * n + 5, pos), packed(Vc, cu3, 2 * n + 5, pos)
    append_packed(pool, Kp, Vp, cu3, pos, n, table)
    append_packed(cache, Kp, Vp, cu3, pos, n)
    lens = [page_rows + n, page_rows + n, 0, 5]
    for counts in ([5, 1, 0, 2], [1, 37, 0, 5]):
        cu = cu_of(counts)
        Qp = packed(Q, cu, cu[-1] + 1)
        got = attend_packed(pool, Qp, cu, lens, max(counts), table)
        assert_bits(f"shared prefix, counts {counts}", got, attend_packed(cache, Qp, cu, lens, max(counts)))
        assert all(np.abs(got[cu[b]:cu[b + 1]]).max() > 0.0 for b in (0, 1, 3))


@pytest.mark.parametrize("page_rows", PAGES)
@pytest.mark.parametrize("variant,d", BUILT)
def test_a_table_entry_outside_the_pool(dev, variant, d, page_rows):
    heads = HEADS[0]
    Q, K, V = dev_inputs(dev, d, heads)
    counts, pos, total, max_n = APPEND_1
    cu = cu_of(counts)
    Kp, Vp = packed(K, cu, total, pos), packed(V, cu, total, pos)
    for bad in (-1, NUM_PAGES, -2 ** 31):
        # append: sequence 3's rows [64, 134) end in the page of row 133
        pool, yard, table = append_setup(dev, variant, d, heads, PCAP, page_rows)
        broken = [list(r) for r in table]
        broken[3][133 // page_rows] = bad
        append_packed(pool, Kp, Vp, cu, pos, max_n, broken)
        pk.yard_append(tokens_append(yard), Kp, Vp, cu, pos, skip=[3])  # nothing of it is written, the tail included
        assert_pool(pool, yard, table, variant, d, heads, page_rows, f"append with entry {bad}")
        # attend: sequence 1 (33 rows) uses its first page only
        acounts, lens = [1, 5, 0, 40], [32, 33, 0, 64]
        acu = cu_of(acounts)
        Qp = packed(Q, acu, 50)
        want = pk.yard_attend(tokens_attend(pool, table), Qp, acu, lens)
        broken = [list(r) for r in table]
        broken[1][0] = bad
        broken[1][1] = bad  # and one behind the used pages, which is not looked at
        broken[0][1] = bad
        got = attend_packed(pool, Qp, acu, lens, 40, broken)
        assert_packed(f"attend with entry {bad}", got, acu, {b: w for b, w in want.items() if b != 1}, zeros=[1])


# ---- 6. a mixed step under graph replay -----------------------------------------------------------------------------------
@pytest.mark.parametrize("page_rows", [None, 64], ids=["contiguous", "paged"])
@pytest.mark.parametrize("variant,d", [(INT8, 64), (F16, 128)])
def test_mixed_step_under_graph_replay(dev, variant, d, page_rows):
    """append_*_packed + attend_*_packed captured once on one side stream (linear) over static tensors, after one eager call
    with every sequence empty; `total` = 44 and the bounds (40) are fixed.  The replays change the mix in device memory: first
    sequence 0 prefills 40 rows while the others decode one row, then all decode, across 32-row group boundaries (sequence 1
    from 30 rows, sequence 3 from 60).  One cu array serves both calls of a step."""
    heads = HEADS[0]
    Q, K, V = dev_inputs(dev, d, heads)
    cap = CAP if page_rows is None else PCAP
    table = None if page_rows is None else TABLES[page_rows]
    start, steps, total, bound = [0, 30, 97, 60], 11, 44, 40
    pc = new_cache(dev, variant, d, heads) if page_rows is None else new_pool(dev, variant, d, heads, page_rows)
    yc = new_cache(dev, variant, d, heads, cap)
    for b, L in enumerate(start):
        if L:
            pos = [0 if i == b else -1 for i in range(B)]
            tokens_append(pc, table)(rows_at(K, pos, L, cap), rows_at(V, pos, L, cap), pos)
            tokens_append(yc)(rows_at(K, pos, L, cap), rows_at(V, pos, L, cap), pos)
    plan, held = [], list(start)
    for k in range(steps):
        counts = [40, 1, 1, 1] if k == 0 else [1, 1, 1, 1]
        plan.append((counts, cu_of(counts), list(held), [held[b] + counts[b] for b in range(B)], [0 if k == 0 else k % NQ] * B))
        held = plan[-1][3]
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    got = []
    with torch.cuda.stream(side):
        qs = torch.zeros((total, Q.shape[2]), dtype=torch.float32, device=dev)
        ks, vs = (torch.zeros((total, K.shape[2]), dtype=torch.float32, device=dev) for _ in range(2))
        buf = torch.full((qs.numel() + 32 * qs.shape[-1],), GUARD, dtype=torch.float32, device=dev)
        out = buf[:qs.numel()].view(qs.shape)
        cu, pos, lens = i32(dev, [0] * (B + 1)), i32(dev, [-1] * B), i32(dev, [0] * B)
        tab = None if table is None else table_dev(dev, table)

        def step():
            if tab is None:
                pc.append_packed(ks, vs, cu, pos, bound)
                pc.attend_packed(qs, cu, lens, bound, out=out)
            else:
                pc.append_paged_packed(ks, vs, cu, pos, tab, bound)
                pc.attend_paged_packed(qs, cu, lens, tab, bound, out=out)

        step()  # both kernels once before the capture; every sequence empty: nothing is read or written
        side.synchronize()
        assert bool((buf == GUARD).all())
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            step()
        for counts, cu_k, pos_k, lens_k, q0 in plan:
            qs.copy_(packed(Q, cu_k, total, q0)), ks.copy_(packed(K, cu_k, total, pos_k)), vs.copy_(packed(V, cu_k, total, pos_k))
            cu.copy_(i32(dev, cu_k)), pos.copy_(i32(dev, pos_k)), lens.copy_(i32(dev, lens_k))
            graph.replay()
            got.append(buf.clone())
        side.synchronize()
    torch.cuda.current_stream(dev).wait_stream(side)
    prev = np.full((total, Q.shape[2]), GUARD, dtype=np.float32)
    for k, (g, (counts, cu_k, pos_k, lens_k, q0)) in enumerate(zip(got, plan)):  # the eager token calls, step by step
        Kp, Vp, Qp = packed(K, cu_k, total, pos_k), packed(V, cu_k, total, pos_k), packed(Q, cu_k, total, q0)
        pk.yard_append(tokens_append(yc), Kp, Vp, cu_k, pos_k)
        want = pk.yard_attend(tokens_attend(yc), Qp, cu_k, lens_k)
        g = g.cpu().numpy()
        assert (g[qs.numel():] == GUARD).all(), "O written past its last row"
        o = g[:qs.numel()].reshape(qs.shape)
        for b in range(B):
            assert_bits(f"replay {k} sequence {b}", o[cu_k[b]:cu_k[b + 1]], want[b])
            assert np.abs(want[b]).max() > 0.0
        assert_bits(f"replay {k}: the rows outside every range keep their bytes", o[cu_k[-1]:], prev[cu_k[-1]:])
        prev = o
    assert held == [50, 41, 108, 71]
    if page_rows is None:
        assert_same_cache("the cache after the loop", pc, yc, variant)
    else:
        assert_pool(pc, yc, table, variant, d, heads, page_rows, "the pool after the loop")


# ---- 7. both bindings -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("heads", [HEADS[0], HEADS[1]], ids=HEAD_IDS[:2])
@pytest.mark.parametrize("variant,d", [(INT8, 64), (F16, 64)])
def test_compiled_binding_gives_the_same_bytes(dev, variant, d, heads):
    Q, K, V = dev_inputs(dev, d, heads)
    mods = (None, compiled_module())
    for page_rows in (None, 64):
        table = None if page_rows is None else TABLES[page_rows]
        caches, outs = [], []
        for mod in mods:
            c = new_cache(dev, variant, d, heads, mod=mod) if page_rows is None else new_pool(dev, variant, d, heads, page_rows, mod=mod)
            c.enable_tokens()  # a second call is a no-op
            for counts, pos, total, max_n in (([31, 0, 0, 64], [0, 0, 0, 0], 95, 64), APPEND_1, APPEND_2):
                cu = cu_of(counts)
                append_packed(c, packed(K, cu, total, pos), packed(V, cu, total, pos), cu, pos, max_n, table)
            counts, total = [1, 5, 0, 40], 50
            cu = cu_of(counts)
            Qp = packed(Q, cu, total)
            outs.append(attend_packed(c, Qp, cu, [39, 73, 3, 164], 40, table))
            args = (i32(dev, cu), i32(dev, [39, 73, 3, 164])) + (() if table is None else (table_dev(dev, table),))
            plain = (c.attend_packed if table is None else c.attend_paged_packed)(Qp, *args, 40)  # without out: zeros outside the ranges
            torch.cuda.synchronize()
            exp = outs[-1].copy()
            exp[exp == GUARD] = 0.0
            assert plain.shape == Qp.shape and np.array_equal(plain.cpu().numpy(), exp)
            caches.append(c)
        assert_same_cache("compiled against ctypes", caches[0], caches[1], variant)
        assert_bits("compiled against ctypes", outs[1], outs[0])
        assert (outs[0][46:] == GUARD).all() and np.abs(outs[0][:46]).max() > 0.0
    cu, lens = i32(dev, [0, 1, 6, 6, 46]), i32(dev, [39, 73, 3, 164])
    Qp, Kp = packed(Q, [0, 1, 6, 6, 46], 50), packed(K, [0, 1, 6, 6, 46], 50)
    for mod in mods:  # dtype, shape and device are checked before the call; int8 needs its tail
        c = new_cache(dev, variant, d, heads, mod=mod, tokens=False)
        if variant == INT8:
            with pytest.raises(RuntimeError, match="needs its tail"):
                c.append_packed(Kp, Kp, cu, lens, 40)
        with pytest.raises(RuntimeError, match="int32"):
            c.attend_packed(Qp, cu.to(torch.int64), lens, 40)
        with pytest.raises(RuntimeError, match="int32"):
            c.attend_packed(Qp, cu, lens.to(torch.int64), 40)
        with pytest.raises(RuntimeError, match="shape"):
            c.attend_packed(Qp, cu[:B], lens, 40)
        with pytest.raises(RuntimeError, match="shape"):
            c.append_packed(Kp, Kp, cu, lens[:2], 40)
        with pytest.raises(RuntimeError, match="CUDA"):
            c.attend_packed(Qp, cu.cpu(), lens, 40)
        with pytest.raises(RuntimeError, match="no batch axis"):
            c.attend_packed(Qp.unsqueeze(0), cu, lens, 40)
        with pytest.raises(RuntimeError, match="out must be"):
            c.attend_packed(Qp, cu, lens, 40, out=torch.empty((49, Qp.shape[1]), dtype=torch.float32, device=dev))
        for bound in (0, 51, CAP + 1):
            with pytest.raises(RuntimeError, match="max_nq"):
                c.attend_packed(Qp, cu, lens, bound)
        p = new_pool(dev, variant, d, heads, 64, mod=mod)
        tab = table_dev(dev, TABLES[64])
        with pytest.raises(RuntimeError, match="shape"):
            p.attend_paged_packed(Qp, cu, lens, tab[:, :3], 40)
        with pytest.raises(RuntimeError, match="max_n"):
            p.append_paged_packed(Kp, Kp, cu, lens, tab, 0)
