"""GPU tests (MI355X) of the sliding-window attends: qmha_attend_cached_tokens_window and
qmha_attend_cached_paged_window through torch_ext's cache classes (ctypes) and the compiled module's.

  1. a window that covers the cache gives attend_tokens / attend_paged bit for bit;
  2. a row that sees nothing of its left tile (Nq = 1 at L % 32 == 0) equals, bit for bit, attend_varlen on the padded block
     over a cache that holds the last `window` rows alone: the sweep starts at first(qg) from the zero state;
  3. O is the restatement (tests/window_ref.py) within the project's bounds (assert_int8, assert_f16);
  4. O is within DESIGN.md 17.1's bounds of float64 band attention on caches built by append_tokens / append_paged alone;
  5. only what is read matters: huge rows before the first staged row and behind ceil32(L), -1 in the table columns behind
     the used ones; a used column outside the pool zeroes that sequence alone;
  6. invalid lengths get positive zeros;
  7. the paged call is the contiguous one bit for bit, with a prefix page shared inside one window and behind another;
  8. a decode loop replayed from a graph equals the eager calls;
  9. the compiled module gives the ctypes classes' bytes and refusals.
Every O is written into the head of a buffer with a sentinel-filled guard behind it.
Shapes: B = 3, cap = 224 (Gk = 7, a partial last stage; paged: 256 logical rows), h = 2 (grouped: h = 4 on h_kv = 2 or 1),
every built (variant, d), pages of 64 and 128 rows under a permuted table, windows 32, 64 and 96.
"""
import functools

import numpy as np
import pytest

from tests import causal_ref as cr
from tests import gpu_support as gs
from tests import window_ref as wr
from tests.gpu_support import BUILT, F16, GUARD, INT8, Guarded, assert_bits, assert_zeros, compiled_module, dev, i32, to_dev  # noqa: F401

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
B, CAP, PCAP, NUM_PAGES, MAX_NQ = wr.B, wr.CAP, 256, 16, 130
HEADS = [(2, None), (4, 2), (4, 1)]  # (h, h_kv); None: multi-head
HEAD_IDS = ["mha", "gqa2", "gqa1"]
TABLES = {64: [[11, 2, 7, 0], [5, 14, 9, 3], [8, 1, 13, 6]], 128: [[11, 2], [5, 14], [8, 1]]}  # permuted, no page twice
# (lens, Nq, windows): decode steps and short blocks at every place of a group; two and three query groups; and five query
# groups in two unit blocks whose waves have different first tiles, some with and some without a left tile
SHAPES = [([33, 95, 224], 1, wr.WINDOWS), ([33, 95, 224], 5, wr.WINDOWS), ([1, 64, 193], 1, wr.WINDOWS), ([1, 64, 193], 5, wr.WINDOWS),
          ([40, 100, 224], 32, wr.WINDOWS), ([40, 100, 224], 40, wr.WINDOWS), ([130, 160, 224], 130, (64,))]


@functools.lru_cache(maxsize=None)
def host_inputs(d, heads):
    """Q [B, MAX_NQ, h d], K, V [B, 256, h_kv d]: the first CAP rows fill a contiguous cache."""
    h, h_kv = heads
    Q = wr.rr.inputs(MAX_NQ, PCAP, h * d, B, "normal", 9800 + d + 10 * h)[0]
    _, K, V = wr.rr.inputs(MAX_NQ, PCAP, (h_kv or h) * d, B, "normal", 9801 + d + (h_kv or 0))
    return Q, K, V


_DEV, _CACHES = {}, {}


@pytest.fixture(scope="module", autouse=True)
def _release_shared_caches():
    """The caches and inputs the tests share live for this module: released while the library can still destroy them."""
    yield
    _CACHES.clear()
    _DEV.clear()


def dev_inputs(dev, d, heads):
    if (d, heads) not in _DEV:
        _DEV[(d, heads)] = to_dev(dev, *host_inputs(d, heads))
    return _DEV[(d, heads)]


def new_cont(dev, variant, d, heads, cap=CAP, nb=B, mod=None):
    c = gs.new_cache(dev, variant, nb, cap, d, *heads, mod=mod)
    c.enable_tokens()
    return c


def new_pool(dev, variant, d, heads, page_rows, mod=None):
    if mod is None:
        from quantizedmha_amd import torch_ext as mod
    h, h_kv = heads
    c = mod.PagedKVCache(B, NUM_PAGES, page_rows, PCAP // page_rows, h * d, h, h_kv, variant, str(dev))
    c.enable_tokens()
    return c


def table_dev(dev, table):
    return torch.tensor(table, dtype=torch.int32, device=dev)


def fill(cache, K, V, lens, table=None, start=None):
    """Sequence b's rows [start[b], lens[b]) (start: 0), one sequence a call (the others left out with pos = -1)."""
    nb = K.shape[0]
    for b, L in enumerate(lens):
        p0 = 0 if start is None else start[b]
        if L - p0 < 1:
            continue
        pos = i32(K.device, [p0 if i == b else -1 for i in range(nb)])
        k, v = (X[b:b + 1, p0:L].expand(nb, L - p0, X.shape[2]).contiguous() for X in (K, V))
        if table is None:
            cache.append_tokens(k, v, pos)
        else:
            cache.append_paged(k, v, pos, table)


def filled(dev, variant, d, heads, kind, lens):
    """A cache of `kind` (0: contiguous, cap 224; 64 / 128: a pool of such pages) holding lens' rows of the shared inputs,
    built once a module: (cache, table or None).  The tests that share it only read it."""
    key = (variant, d, heads, kind, tuple(lens))
    if key not in _CACHES:
        _, K, V = dev_inputs(dev, d, heads)
        table = table_dev(dev, TABLES[kind]) if kind else None
        cache = new_pool(dev, variant, d, heads, kind) if kind else new_cont(dev, variant, d, heads)
        fill(cache, K, V, lens, table)
        _CACHES[key] = (cache, table)
    return _CACHES[key]


def attend(cache, Q, lens, window=None, table=None):
    """attend_tokens / attend_paged (window None) or their windowed forms, through the guard: O (numpy) after a sync."""
    g = Guarded(Q)
    ln = i32(Q.device, lens)
    if table is None:
        cache.attend_tokens(Q, ln, out=g.buf[:g.n]) if window is None else cache.attend_tokens_window(Q, ln, window, out=g.buf[:g.n])
    else:
        cache.attend_paged(Q, ln, table, out=g.buf[:g.n]) if window is None else cache.attend_paged_window(Q, ln, table, window, out=g.buf[:g.n])
    return g.result()


# ---- 1. a window that covers the cache ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("heads", HEADS, ids=HEAD_IDS)
@pytest.mark.parametrize("variant,d", BUILT)
def test_a_covering_window_is_the_unwindowed_call(dev, variant, d, heads):
    Q = dev_inputs(dev, d, heads)[0]
    for lens, Nq, _ in SHAPES:
        q = Q[:, :Nq].contiguous()
        for kind, cover in ((0, (CAP, 2 ** 31 - 32)), (64, (PCAP,)), (128, (PCAP,))):
            cache, table = filled(dev, variant, d, heads, kind, lens)
            want = attend(cache, q, lens, None, table)
            for window in cover:
                assert_bits(f"{variant} d{d} {heads} pages {kind} lens {lens} Nq {Nq} window {window}", attend(cache, q, lens, window, table), want)
            assert all(np.abs(want[b]).max() > 0.0 for b, L in enumerate(lens) if L >= Nq)


# ---- 2. a row that sees nothing of its left tile ------------------------------------------------------------------------------
def last_rows_cache(cache, small, b, L, window):
    """The quantised bytes of sequence b's rows [L - window, L), copied group by group to row 0 on of `small` (B = 1,
    cap = window): every array of the carve holds a slice's 32-row groups back to back."""
    hk = cache.num_kv_heads
    g1 = L // 32
    g0 = g1 - window // 32
    small.mem.zero_()
    for name in gs.cache_layout(cache):
        src = gs.cache_array(cache, name, torch.uint8)[b * hk:(b + 1) * hk]
        dst = gs.cache_array(small, name, torch.uint8)
        pg = src.shape[1] // (cache.cap // 32)  # bytes of a group
        assert pg * (cache.cap // 32) == src.shape[1] and dst.shape[1] == pg * (window // 32), name
        dst[:, :] = src[:, g0 * pg:g1 * pg]


@pytest.mark.parametrize("heads", HEADS, ids=HEAD_IDS)
@pytest.mark.parametrize("variant,d", BUILT)
def test_a_row_that_sees_nothing_of_its_left_tile(dev, variant, d, heads):
    """Nq = 1 at L % 32 == 0: the real row is slot 31 of its group, which the left tile's mask (c > r) leaves no key.  Its
    tiles after the left one are the last `window` rows, which it sees whole, from a state the left tile left at zero."""
    Q = dev_inputs(dev, d, heads)[0]
    lens = [64, 128, 224]
    cache, _ = filled(dev, variant, d, heads, 0, lens)
    q = Q[:, :1].contiguous()
    for window in (32, 64):
        got = attend(cache, q, lens, window)
        small = gs.new_cache(dev, variant, 1, window, d, *heads)
        for b, L in enumerate(lens):
            last_rows_cache(cache, small, b, L, window)
            blk = torch.zeros((1, 32, q.shape[2]), dtype=torch.float32, device=dev)
            blk[0, 31] = q[b, 0]
            want = gs.attend(small, blk, causal=True, lens=i32(dev, [window]))
            assert_bits(f"{variant} d{d} {heads} L {L} window {window}", got[b, 0], want[0, 31])
            assert np.abs(want[0, 31]).max() > 0.0


# ---- 3. against the restatement -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("heads", HEADS, ids=HEAD_IDS)
@pytest.mark.parametrize("variant,d", BUILT)
def test_against_the_restatement(dev, oracle_mod, variant, d, heads):
    Qd = dev_inputs(dev, d, heads)[0]
    Q, K, V = host_inputs(d, heads)
    h, h_kv = heads[0], heads[1] or heads[0]
    for lens, Nq, windows in SHAPES:
        cache, _ = filled(dev, variant, d, heads, 0, lens)
        q = Qd[:, :Nq].contiguous()
        for window in windows:
            got = attend(cache, q, lens, window)
            for b, L in enumerate(lens):
                label = f"{variant} d{d} {heads} lens {lens} Nq {Nq} window {window} sequence {b}"
                if L < Nq:
                    assert_zeros(label, got[b])
                    continue
                ref, unit = wr.attend(oracle_mod, variant, Q[b, :Nq], K[b], V[b], L, h, h_kv, window)
                if variant == INT8:
                    gs.assert_int8(label, got[b], ref, unit, " window")
                else:
                    gs.assert_f16(label, got[b], ref, cr.fp16_lazy_tol(CAP), " window")


# ---- 4. against float64 -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def float64_cases():
    return wr.float64_inputs(tuple(BUILT))


@pytest.mark.parametrize("paged", [False, True], ids=["contiguous", "paged"])
@pytest.mark.parametrize("variant,d", BUILT)
def test_against_float64(dev, variant, d, paged):
    """Caches built by append_tokens / append_paged alone; int8 within 5e-3, fp16 within max(1e-3, 1e-3 |ref|) of float64 band
    attention (tests/test_window_cpu.py holds the restatement to the same bounds on the same inputs)."""
    ran, worst, built = 0, 0.0, {}
    for label, v, dd, h, h_kv, window, lens, Nq, Q, K, V in float64_cases():
        if (v, dd) != (variant, d):
            continue
        heads = (h, None if h_kv == h else h_kv)
        key = (h, h_kv, tuple(lens), Nq, label.split(" ")[3])
        if key not in built:
            q, k, v_ = to_dev(dev, Q, K, V)
            table = table_dev(dev, TABLES[64]) if paged else None
            cache = new_pool(dev, variant, d, heads, 64) if paged else new_cont(dev, variant, d, heads)
            fill(cache, k, v_, lens, table)
            built[key] = (cache, table, q)
        cache, table, q = built[key]
        O = attend(cache, q, lens, window, table)
        for b, L in enumerate(lens):
            ref = wr.attention_f64(Q[b], K[b], V[b], L, h, h_kv, window)
            err = float(np.abs(O[b] - ref).max())
            worst = max(worst, err)
            assert wr.within_bound(variant, O[b], ref), (label, b, err)
        ran += 1
    print(f"{variant} d{d} {'paged' if paged else 'contiguous'}: worst |gpu - float64| = {worst:.3e} over {ran} cases")
    assert ran >= 12


# ---- 5. only what is read matters -----------------------------------------------------------------------------------------------
GARBAGE = [([95, 193, 224], 5, 32), ([95, 193, 224], 5, 64), ([100, 160, 224], 40, 96), ([130, 160, 224], 130, 64)]


@pytest.mark.parametrize("variant,d", BUILT)
def test_rows_outside_the_staged_range_do_not_matter(dev, variant, d):
    """Rows of magnitude 1e30 in every cache row before 64 * (first(0) / 2) and behind ceil32(L): O is the clean run's."""
    Q, K, V = dev_inputs(dev, d, HEADS[0])
    huge_k, huge_v = torch.full_like(K[:, :CAP], 1e30), torch.full_like(V[:, :CAP], -1e30)
    for lens, Nq, window in GARBAGE:
        q = Q[:, :Nq].contiguous()
        clean, _ = filled(dev, variant, d, HEADS[0], 0, lens)
        want = attend(clean, q, lens, window)
        dirty = new_cont(dev, variant, d, HEADS[0])
        dirty.append_tokens(huge_k, huge_v, i32(dev, [0] * B))  # everywhere; fill() then rewrites the groups below ceil32(L)
        fill(dirty, K, V, lens)
        lo = [wr.first_row_staged(L, Nq, window) for L in lens]
        fill(dirty, huge_k, huge_v, lo)  # rows [0, lo): whole groups, behind the first stage the call brings in
        got = attend(dirty, q, lens, window)
        assert np.isfinite(got).all()
        assert_bits(f"{variant} d{d} lens {lens} Nq {Nq} window {window} lo {lo}", got, want)
    assert any(x > 0 for _, Nq, w in GARBAGE[:2] for x in [wr.first_row_staged(224, Nq, w)])


@pytest.mark.parametrize("page_rows", [64, 128])
@pytest.mark.parametrize("variant,d", BUILT)
def test_table_columns_behind_the_window_are_not_read(dev, variant, d, page_rows):
    Q = dev_inputs(dev, d, HEADS[1])[0]
    hidden = 0
    for lens, Nq, window in GARBAGE:
        q = Q[:, :Nq].contiguous()
        cont, _ = filled(dev, variant, d, HEADS[1], 0, lens)
        pool, table = filled(dev, variant, d, HEADS[1], page_rows, lens)
        want = attend(cont, q, lens, window)
        behind = table.clone()
        for b, L in enumerate(lens):
            ncol = wr.first_row_staged(L, Nq, window) // page_rows  # columns wholly behind the first staged row
            behind[b, :ncol] = -1
            hidden += ncol
        label = f"{variant} d{d} pages {page_rows} lens {lens} Nq {Nq} window {window}"
        assert_bits(label + ": -1 behind the window", attend(pool, q, lens, window, behind), want)
        # a used column outside the pool: the column of the last row of sequence 1
        broken = behind.clone()
        broken[1, (lens[1] - 1) // page_rows] = NUM_PAGES
        got = attend(pool, q, lens, window, broken)
        assert_zeros(label + ": a used entry outside the pool", got[1])
        assert_bits(label + ": the others", got[[0, 2]], want[[0, 2]])
        broken = behind.clone()  # ... and the column of the first staged row
        broken[1, wr.first_row_staged(lens[1], Nq, window) // page_rows] = -1
        assert_zeros(label + ": the first used entry is -1", attend(pool, q, lens, window, broken)[1])
    assert hidden > 0


# ---- 6. invalid lengths -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("heads", [HEADS[0], HEADS[2]], ids=["mha", "gqa1"])
@pytest.mark.parametrize("variant,d", BUILT)
def test_invalid_lengths_get_zeros(dev, variant, d, heads):
    Q = dev_inputs(dev, d, heads)[0]
    q = Q[:, :5].contiguous()
    for kind in (0, 64):
        cache, table = filled(dev, variant, d, heads, kind, [33, 100, 224])
        for window in (32, 64):
            want = attend(cache, q, [33, 100, 224], window, table)
            got = attend(cache, q, [0, 100, 300], window, table)
            assert_zeros("lens 0", got[0]), assert_zeros("lens 300 > cap", got[2])
            assert_bits("the valid sequence", got[1], want[1])
            assert np.abs(want[1]).max() > 0.0
            assert_zeros("lens 4 < Nq", attend(cache, q, [4, 100, 224], window, table)[0])


# ---- 7. paged is contiguous -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("page_rows", [64, 128])
@pytest.mark.parametrize("heads", HEADS, ids=HEAD_IDS)
@pytest.mark.parametrize("variant,d", BUILT)
def test_paged_is_contiguous(dev, variant, d, heads, page_rows):
    Q = dev_inputs(dev, d, heads)[0]
    for lens, Nq, windows in SHAPES:
        cont, _ = filled(dev, variant, d, heads, 0, lens)
        pool, table = filled(dev, variant, d, heads, page_rows, lens)
        q = Q[:, :Nq].contiguous()
        for window in windows:
            assert_bits(f"paged against contiguous, lens {lens} Nq {Nq} window {window}", attend(pool, q, lens, window, table),
                        attend(cont, q, lens, window))


@pytest.mark.parametrize("variant,d", BUILT)
def test_a_shared_prefix_page_inside_one_window_and_behind_another(dev, variant, d):
    """Sequences 0, 1 and 2 name the same first page, written once through sequence 0.  At window 64 and Nq = 1 sequence 0
    (101 rows) stages from row 0 on -- the page is used --, sequence 1 (224 rows) from row 128 on: for it the page lies behind
    the window, and its column may as well hold -1."""
    Q, K, V = dev_inputs(dev, d, HEADS[0])
    page_rows, window = 64, 64
    lens = [101, 224, 101]
    Kc, Vc = K.clone(), V.clone()
    for b in (1, 2):
        Kc[b, :page_rows], Vc[b, :page_rows] = K[0, :page_rows], V[0, :page_rows]  # the contiguous cache holds the prefix thrice
    table = table_dev(dev, TABLES[page_rows])
    table[1, 0] = table[2, 0] = table[0, 0]
    cont, pool = new_cont(dev, variant, d, HEADS[0]), new_pool(dev, variant, d, HEADS[0], page_rows)
    fill(cont, Kc, Vc, lens)
    fill(pool, Kc, Vc, [page_rows, 0, 0], table)  # the prefix, through sequence 0
    fill(pool, Kc, Vc, lens, table, start=[page_rows] * B)
    assert wr.first_row_staged(lens[0], 1, window) == 0 and wr.first_row_staged(lens[1], 1, window) == 128
    for Nq in (1, 5):
        q = Q[:, :Nq].contiguous()
        want = attend(cont, q, lens, window)
        assert_bits(f"shared prefix Nq {Nq}", attend(pool, q, lens, window, table), want)
        gone = table.clone()
        gone[1, 0] = -1
        assert_bits(f"shared prefix Nq {Nq}, behind sequence 1's window", attend(pool, q, lens, window, gone), want)


# ---- 8. a decode loop under graph replay ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("paged", [False, True], ids=["contiguous", "paged"])
@pytest.mark.parametrize("variant,d", [(INT8, 64), (F16, 128)])
def test_decode_loop_under_graph_replay(dev, variant, d, paged):
    """One append (n = 1) and one windowed attend (Nq = 1, window 64) captured once on a side stream (single stream, linear)
    over static tensors; 35 replays, between which the new K, V, Q rows are copied in and pos / lens advance by 1 on that
    stream.  Sequences 0 and 1 start at 30 and 97 rows: sequence 0 crosses a tile and a stage boundary and gets its first left
    tile (L = 65), sequence 1 moves its first tile and its first stage (and, paged, ends in a new page).  Sequence 2 is an
    empty slot.  Every replay equals the eager call on a cache of its own."""
    window, page_rows = 64, 64
    Q, K, V = dev_inputs(dev, d, HEADS[0])
    start, steps = [30, 97], 35
    table = table_dev(dev, TABLES[page_rows]) if paged else None
    make = (lambda: new_pool(dev, variant, d, HEADS[0], page_rows)) if paged else (lambda: new_cont(dev, variant, d, HEADS[0], cap=PCAP))
    cache, yard = make(), make()
    fill(cache, K, V, start + [0], table), fill(yard, K, V, start + [0], table)
    append = (lambda c, k, v, p: c.append_paged(k, v, p, table)) if paged else (lambda c, k, v, p: c.append_tokens(k, v, p))
    att = (lambda c, q, ln, out: c.attend_paged_window(q, ln, table, window, out=out)) if paged else \
        (lambda c, q, ln, out: c.attend_tokens_window(q, ln, window, out=out))
    row = lambda X, rows: torch.stack([X[b, max(r, 0):max(r, 0) + 1] for b, r in enumerate(rows)]).contiguous()  # noqa: E731
    qrow = lambda k: torch.stack([Q[b, k % MAX_NQ:k % MAX_NQ + 1] for b in range(B)]).contiguous()  # noqa: E731
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    got = []
    with torch.cuda.stream(side):
        qs = torch.zeros((B, 1, Q.shape[2]), dtype=torch.float32, device=dev)
        ks, vs = (torch.zeros((B, 1, K.shape[2]), dtype=torch.float32, device=dev) for _ in range(2))
        buf = torch.full((qs.numel() + 32 * qs.shape[-1],), GUARD, dtype=torch.float32, device=dev)
        pos, lens = i32(dev, [-1] * B), i32(dev, [0] * B)
        append(cache, ks, vs, pos)  # every kernel once before the capture; every sequence invalid: nothing is placed
        att(cache, qs, lens, buf[:qs.numel()])
        pos.copy_(i32(dev, start + [-1]))
        lens.copy_(i32(dev, [L + 1 for L in start] + [0]))
        inc = i32(dev, [1, 1, 0])
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            append(cache, ks, vs, pos)
            att(cache, qs, lens, buf[:qs.numel()])
        for k in range(steps):
            rows = [L + k for L in start] + [0]
            qs.copy_(qrow(k)), ks.copy_(row(K, rows)), vs.copy_(row(V, rows))
            graph.replay()
            got.append(buf.clone())
            pos.add_(inc), lens.add_(inc)
        side.synchronize()
    torch.cuda.current_stream(dev).wait_stream(side)
    assert pos.tolist() == [30 + steps, 97 + steps, -1]
    firsts = [{wr.first_row_staged(L + k + 1, 1, window) for k in range(steps)} for L in start]
    assert len(firsts[0]) == 1 and len(firsts[1]) == 2  # sequence 1's first stage moves during the loop
    assert {wr.first_tile(L + k + 1, 1, window) for L in start for k in range(steps)} >= {0, 1, 2}
    for k, g in enumerate(got):  # the eager path, step by step
        rows = [L + k for L in start] + [-1]
        append(yard, row(K, rows), row(V, rows), i32(dev, rows))
        gd = Guarded(qs)
        att(yard, qrow(k), i32(dev, [L + k + 1 for L in start] + [0]), gd.buf[:gd.n])
        want = gd.result()
        g = g.cpu().numpy()
        assert (g[qs.numel():] == GUARD).all(), "O written past its last row"
        o = g[:qs.numel()].reshape(qs.shape)
        assert_bits(f"replay {k}", o[:2], want[:2])
        assert np.abs(o[:2]).max() > 0.0
        assert_zeros(f"replay {k}: the empty slot", o[2])


# ---- 9. both bindings -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("heads", [HEADS[0], HEADS[1]], ids=HEAD_IDS[:2])
@pytest.mark.parametrize("variant,d", [(INT8, 64), (F16, 64)])
def test_compiled_binding_gives_the_same_bytes(dev, variant, d, heads):
    Q, K, V = dev_inputs(dev, d, heads)
    q = Q[:, :5].contiguous()
    lens = [45, 171, 0]
    table = table_dev(dev, TABLES[64])
    for paged in (False, True):
        for window in (32, 96):
            outs = []
            for mod in (None, compiled_module()):
                c = new_pool(dev, variant, d, heads, 64, mod=mod) if paged else new_cont(dev, variant, d, heads, mod=mod)
                fill(c, K, V, lens, table if paged else None)
                outs.append(attend(c, q, lens, window, table if paged else None))
                plain = c.attend_paged_window(q, i32(dev, lens), table, window) if paged else c.attend_tokens_window(q, i32(dev, lens), window)
                torch.cuda.synchronize()
                assert plain.shape == q.shape and np.array_equal(plain.cpu().numpy(), outs[-1])
            assert_bits("compiled against ctypes", outs[1], outs[0])
            assert_zeros("the empty slot", outs[0][2])
            assert np.abs(outs[0][:2]).max() > 0.0
    for mod in (None, compiled_module()):  # the refusals
        c, p = new_cont(dev, variant, d, heads, mod=mod), new_pool(dev, variant, d, heads, 64, mod=mod)
        for bad in (0, -32, 31, 48):
            with pytest.raises(RuntimeError, match="multiple of 32 with window >= 32"):
                c.attend_tokens_window(q, i32(dev, lens), bad)
            with pytest.raises(RuntimeError, match="multiple of 32 with window >= 32"):
                p.attend_paged_window(q, i32(dev, lens), table, bad)
        with pytest.raises(RuntimeError, match="int32"):
            c.attend_tokens_window(q, i32(dev, lens).to(torch.int64), 64)
        with pytest.raises(RuntimeError, match="int32"):
            p.attend_paged_window(q, i32(dev, lens), table.to(torch.int64), 64)
        with pytest.raises(RuntimeError):
            c.attend_tokens_window(q[:, :, :-1].contiguous(), i32(dev, lens), 64)
