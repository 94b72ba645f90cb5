"""GPU tests (MI355X) of the split-KV attend: qmha_attend_cached_tokens_split and
qmha_attend_cached_paged_split through torch_ext's cache classes (ctypes) and the compiled module's.

The split call is a deterministic function of its own, defined so that it can be held to kernels that already ship:
  1. every partial the combine reads is, bit for bit, attend_varlen on the group's zero-padded 32-row Q block over a cache
     that holds that chunk's rows alone;
  2. O is the float64 evaluation of the combine formula on the fp32 partials, within (2 n_c + 4) 2^-23 max|Oc|;
  3. only what is read matters (NaN scratch, huge K/V rows behind ceil32(L), a sentinel behind the scratch);
  4. invalid sequences get positive zeros and leave their scratch alone;
  5. O is within the contract of DESIGN.md 17.1 of float64, on caches built by append_tokens / append_paged alone;
  6. the paged call is the contiguous one, bit for bit, in O and in the partials;
  7. a decode loop replayed from a graph equals the eager calls;
  8. the compiled module gives the ctypes classes' bytes and refusals;
  9. one chunk (chunk_rows >= ceil64(L)) is attend_tokens within the combine's rounding.
Every O is written into the head of a buffer with a sentinel-filled guard behind it.
Shapes: B = 3, cap = 224 (the last stage and the last chunk are partial; paged: 256 logical rows), chunk_rows 64 and 128,
h = 2 (grouped: h = 4 on h_kv = 2 or 1), every built (variant, d), pages of 64 and 128 rows under a permuted table.
"""
import functools

import numpy as np
import pytest

from tests import gpu_support as gs
from tests import split_ref as sr
from tests.gpu_support import BUILT, F16, GUARD, INT8, Guarded, assert_bits, assert_zeros, compiled_module, dev, i32, to_dev  # noqa: F401

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
B, CAP, PCAP, NUM_PAGES, MAX_NQ = sr.B, sr.CAP, 256, 16, 40
HEADS = [(2, None), (4, 2), (4, 1)]  # (h, h_kv); None: multi-head
HEAD_IDS = ["mha", "gqa2", "gqa1"]
TABLES = {64: [[11, 2, 7, 0], [5, 14, 9, 3], [8, 1, 13, 6]], 128: [[11, 2], [5, 14], [8, 1]]}  # permuted, no page twice
# (lens, Nq): decode steps and short blocks at every place of a group; Nq = 32 at s != 0 (two query groups) and 40 (three),
# where the masked region crosses a chunk boundary
SHAPES = [([33, 95, 224], 1), ([33, 95, 224], 5), ([1, 64, 193], 1), ([1, 64, 193], 5), ([40, 100, 224], 32), ([40, 100, 224], 40)]


@functools.lru_cache(maxsize=None)
def host_inputs(d, heads, dist="normal"):
    """Q [B, MAX_NQ, h d], K, V [B, 256, h_kv d]: the first CAP rows fill a contiguous cache."""
    h, h_kv = heads
    Q = sr.rr.inputs(MAX_NQ, PCAP, h * d, B, dist, 9700 + d + 10 * h)[0]
    _, K, V = sr.rr.inputs(MAX_NQ, PCAP, (h_kv or h) * d, B, dist, 9701 + d + (h_kv or 0))
    return Q, K, V


_DEV = {}


def dev_inputs(dev, d, heads):
    if (d, heads) not in _DEV:
        _DEV[(d, heads)] = to_dev(dev, *host_inputs(d, heads))
    return _DEV[(d, heads)]


def new_cont(dev, variant, d, heads, chunk, cap=CAP, nb=B, mod=None):
    c = gs.new_cache(dev, variant, nb, cap, d, *heads, mod=mod)
    c.enable_tokens()
    if chunk:
        c.enable_split(chunk, MAX_NQ)
    return c


def new_pool(dev, variant, d, heads, page_rows, chunk, mod=None):
    if mod is None:
        from quantizedmha_amd import torch_ext as mod
    h, h_kv = heads
    c = mod.PagedKVCache(B, NUM_PAGES, page_rows, PCAP // page_rows, h * d, h, h_kv, variant, str(dev))
    c.enable_tokens()
    c.enable_split(chunk, MAX_NQ)
    return c


def table_dev(dev, table):
    return torch.tensor(table, dtype=torch.int32, device=dev)


def fill(cache, K, V, lens, table=None):
    """Sequence b's first lens[b] rows, one sequence a call (the others left out with pos = -1), by append_tokens / append_paged."""
    nb = K.shape[0]
    for b, L in enumerate(lens):
        if L < 1:
            continue
        pos = i32(K.device, [0 if i == b else -1 for i in range(nb)])
        k, v = (X[b:b + 1, :L].expand(nb, L, X.shape[2]).contiguous() for X in (K, V))
        if table is None:
            cache.append_tokens(k, v, pos)
        else:
            cache.append_paged(k, v, pos, table)


def split_attend(cache, Q, lens, table=None):
    """The split attend through the guard: O (numpy) after a sync."""
    g = Guarded(Q)
    if table is None:
        cache.attend_tokens_split(Q, i32(Q.device, lens), out=g.buf[:g.n])
    else:
        cache.attend_paged_split(Q, i32(Q.device, lens), table, out=g.buf[:g.n])
    return g.result()


def partials(cache, Nq):
    torch.cuda.synchronize()
    return [x.cpu().numpy().copy() for x in cache.split_partials(Nq)]


def chunk_cache_of(cache, chunk_cache, b, c, chunk):
    """The quantised bytes of sequence b's rows [c chunk, c chunk + chunk) (those the cache has), copied group by group to
    row 0 on of `chunk_cache` (B = 1, cap = chunk): every array of the carve holds a slice's 32-row groups back to back."""
    hk = cache.num_kv_heads
    g0 = c * chunk // 32
    g1 = min(g0 + chunk // 32, cache.cap // 32)
    chunk_cache.mem.zero_()
    for name in gs.cache_layout(cache):
        src = gs.cache_array(cache, name, torch.uint8)[b * hk:(b + 1) * hk]
        dst = gs.cache_array(chunk_cache, name, torch.uint8)
        pg = src.shape[1] // (cache.cap // 32)  # bytes of a group
        assert pg * (cache.cap // 32) == src.shape[1] and dst.shape[1] == pg * (chunk // 32), name
        dst[:, :(g1 - g0) * pg] = src[:, g0 * pg:g1 * pg]


def check_partials(cache, chunk_cache, Q, lens, chunk, Oc, label):
    """1.: every (sequence, query group, chunk) the combine reads, against attend_varlen on the chunk's rows alone."""
    Nq, C = Q.shape[1], chunk // 32
    checked = 0
    for b, L in enumerate(lens):
        if L < Nq:  # an invalid sequence: no partial
            continue
        s, Nqp, Lp, off, _ = sr.geometry(L, Nq, chunk)
        for qg in range(Nqp // 32):
            rows = np.arange(qg * 32, qg * 32 + 32) - s
            real = (rows >= 0) & (rows < Nq)
            blk = torch.zeros((1, 32, Q.shape[2]), dtype=torch.float32, device=Q.device)
            blk[0, torch.from_numpy(np.nonzero(real)[0]).to(Q.device)] = Q[b, torch.from_numpy(rows[real]).to(Q.device)]
            diag = qg + off
            for c in range(diag // C + 1):
                chunk_cache_of(cache, chunk_cache, b, c, chunk)
                if c * C + C - 1 >= diag:  # the chunk holds the group's diagonal tile: its last
                    want = gs.attend(chunk_cache, blk, causal=True, lens=i32(Q.device, [32 * (diag + 1) - 32 * c * C]))
                else:
                    want = gs.attend(chunk_cache, blk, causal=False, lens=i32(Q.device, [chunk]))
                assert_bits(f"{label} sequence {b} L {L} group {qg} chunk {c}", Oc[b, c, rows[real]], want[0, real])
                checked += 1
    return checked


# ---- 1. partials are the shipped kernel's bits; 2. the combine ----------------------------------------------------------------
@pytest.mark.parametrize("chunk", sr.CHUNKS)
@pytest.mark.parametrize("heads", HEADS, ids=HEAD_IDS)
@pytest.mark.parametrize("variant,d", BUILT)
def test_partials_are_the_shipped_kernels_bits_and_o_is_their_combination(dev, variant, d, heads, chunk):
    """1. Oc of every chunk the combine reads equals attend_varlen's bits on that chunk's rows alone.
    2. O equals the float64 evaluation of DESIGN.md 19.2 on the fp32 partials read back, per element within
    (2 n_c + 4) 2^-23 max_c |Oc_c| over the row's n_c chunks: v_exp_f32 is good to one ulp, so a weight a_c carries 1.5
    ulp (exp2, the product with l_c); a term a_c Oc_c and its accumulation add half an ulp each, n_c terms; Ltot's n_c
    additions half an ulp each; the division half an ulp -- relative to sum a_c |Oc_c| / Ltot <= max |Oc_c|, under
    (2 n_c + 4) ulp in all."""
    Q, K, V = dev_inputs(dev, d, heads)
    chunk_cache = new_cont(dev, variant, d, heads, None, cap=chunk, nb=1)
    checked = 0
    for lens, Nq in SHAPES:
        cache = new_cont(dev, variant, d, heads, chunk)
        fill(cache, K, V, lens)
        q = Q[:, :Nq].contiguous()
        O = split_attend(cache, q, lens)
        Oc, pm, pl = partials(cache, Nq)
        label = f"{variant} d{d} {heads} chunk {chunk} lens {lens} Nq {Nq}"
        checked += check_partials(cache, chunk_cache, q, lens, chunk, Oc, label)
        for b, L in enumerate(lens):
            if L < Nq:  # lens [1, 64, 193] at Nq = 5: sequence 0 is invalid
                assert_zeros(f"{label} sequence {b} (invalid)", O[b])
                continue
            want, bound = sr.combine_f64(Oc[b], pm[b], pl[b], sr.chunks_read(L, Nq, chunk), sr.THR[variant])
            err = np.abs(O[b].astype(np.float64) - want)
            print(f"{label} sequence {b}: worst |O - float64 combine| / bound = {float((err / np.maximum(bound, 1e-300)).max()):.3f}")
            assert np.isfinite(O[b]).all() and (err <= bound).all(), (label, b, float(err.max()))
            assert np.abs(O[b]).max() > 0.0
    assert checked >= 30  # (sequence, query group, chunk) triples: 33 at chunks of 128 rows, more at 64


@pytest.mark.parametrize("variant,d,name", sr.HARD_COMBINE)
def test_combine_over_climbing_maxima(dev, oracle_mod, variant, d, name):
    """The staircase: the chunks' m climb by more than 128 log2 units, where a combine around a stale maximum overflows."""
    Q, K, V, h = sr.hard_inputs(name, d)
    q, k, v = to_dev(dev, Q[None], K[None], V[None])
    for chunk in sr.CHUNKS:
        cache = new_cont(dev, variant, d, (h, None), chunk, cap=sr.HARD_CAP, nb=1)
        fill(cache, k, v, [sr.HARD_CAP])
        O = split_attend(cache, q, [sr.HARD_CAP])
        Oc, pm, pl = partials(cache, sr.HARD_NQ)
        reads = sr.chunks_read(sr.HARD_CAP, sr.HARD_NQ, chunk)
        assert float((pm[0, :reads.max()].max(axis=0) - pm[0, :reads.max()].min(axis=0)).min()) > 128.0
        want, bound = sr.combine_f64(Oc[0], pm[0], pl[0], reads, sr.THR[variant])
        assert np.isfinite(O).all() and (np.abs(O[0] - want) <= bound).all(), (chunk, float(np.abs(O[0] - want).max()))


# ---- 3. only what is read matters ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk", sr.CHUNKS)
@pytest.mark.parametrize("variant,d", BUILT)
def test_only_what_is_read_matters(dev, variant, d, chunk):
    Q, K, V = dev_inputs(dev, d, HEADS[0])
    for lens, Nq in (([33, 95, 193], 5), ([40, 100, 160], 40)):
        q = Q[:, :Nq].contiguous()
        outs = []
        for dirty in (False, True):
            cache = new_cont(dev, variant, d, HEADS[0], chunk)
            if dirty:  # rows of magnitude 1e30 everywhere; append_tokens then rewrites the groups below ceil32(L) only
                cache.append_tokens(torch.full_like(K[:, :CAP], 1e30), torch.full_like(V[:, :CAP], -1e30), i32(dev, [0] * B))
            fill(cache, K, V, lens)
            cache.split_scratch.fill_(0xFF if dirty else 0)  # NaN bytes / zeros
            outs.append(split_attend(cache, q, lens))
            if dirty:  # the scratch behind qmha_attend_split_bytes(Nq) keeps its sentinel (it is sized for MAX_NQ rows)
                from quantizedmha_amd import _lib
                used = _lib.load().qmha_attend_split_bytes(cache._handle, Nq, chunk)
                assert 0 < used <= cache.split_scratch.numel()
                assert bool((cache.split_scratch[used:] == 0xFF).all()), "the scratch was written behind qmha_attend_split_bytes"
        assert np.isfinite(outs[1]).all()
        assert_bits(f"dirty cache and NaN scratch, lens {lens} Nq {Nq}", outs[1], outs[0])
        assert all(np.abs(outs[0][b]).max() > 0.0 for b in range(B))


# ---- 4. invalid sequences -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk", sr.CHUNKS)
@pytest.mark.parametrize("heads", [HEADS[0], HEADS[2]], ids=["mha", "gqa1"])
@pytest.mark.parametrize("variant,d", BUILT)
def test_invalid_sequences_get_zeros_and_leave_their_scratch(dev, variant, d, heads, chunk):
    Q, K, V = dev_inputs(dev, d, heads)
    q = Q[:, :5].contiguous()
    cache = new_cont(dev, variant, d, heads, chunk)
    fill(cache, K, V, [33, 100, 224])
    want = split_attend(cache, q, [33, 100, 224])
    want_parts = partials(cache, 5)
    cache.split_scratch.fill_(0xFF)
    got = split_attend(cache, q, [0, 100, 300])
    parts = partials(cache, 5)
    assert_zeros("lens 0", got[0]), assert_zeros("lens 300 > cap", got[2])
    assert_bits("the valid sequence", got[1], want[1])
    reads = sr.chunks_read(100, 5, chunk).max()
    for x, w in zip(parts, want_parts):
        assert np.isnan(x[0]).all() and np.isnan(x[2]).all(), "an invalid sequence's scratch was written"
        assert_bits("the valid sequence's partials", x[1, :reads], w[1, :reads])
        assert np.isnan(x[1, reads:]).all(), "a chunk the sequence does not reach was written"
    # a used table entry outside the pool
    pool = new_pool(dev, variant, d, heads, 64, chunk)
    table = table_dev(dev, TABLES[64])
    fill(pool, K, V, [33, 100, 224], table)
    for bad in (-1, NUM_PAGES, -2 ** 31):
        broken = table.clone()
        broken[1, 1] = bad
        pool.split_scratch.fill_(0xFF)
        got = split_attend(pool, q, [33, 100, 224], broken)
        assert_zeros(f"entry {bad}", got[1])
        assert_bits(f"entry {bad}: the others", got[[0, 2]], want[[0, 2]])
        assert all(np.isnan(x[1]).all() for x in partials(pool, 5)), "an invalid sequence's scratch was written"


# ---- 5. against float64 ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def float64_cases():
    return sr.float64_inputs(tuple(BUILT))


@pytest.mark.parametrize("paged", [False, True], ids=["contiguous", "paged"])
@pytest.mark.parametrize("variant,d", BUILT)
def test_against_float64(dev, variant, d, paged):
    """Caches built by append_tokens / append_paged alone; int8 within 5e-3, fp16 within max(1e-3, 1e-3 |ref|) of float64
    attention (tests/test_split_cpu.py holds the restatement to the same bounds on the same inputs).  The fp16 d = 128 run
    includes the ramp, whose chunk maxima climb by more than 48 log2 units."""
    ran = 0
    for label, v, h, h_kv, chunk, seqs, cap in float64_cases():
        if (v, int(seqs[0][0].shape[1]) // h) != (variant, d):
            continue
        nb = len(seqs)
        q, k, v_ = to_dev(dev, np.stack([s[0] for s in seqs]), np.stack([s[1] for s in seqs]), np.stack([s[2] for s in seqs]))
        lens = [s[3] for s in seqs]
        if paged:
            if cap != CAP:
                continue  # the pool's logical capacity is 256 rows
            cache = new_pool(dev, variant, d, (h, h_kv), 64, chunk)
            table = table_dev(dev, TABLES[64])
            fill(cache, k, v_, lens, table)
            O = split_attend(cache, q, lens, table)
        else:
            cache = new_cont(dev, variant, d, (h, h_kv), chunk, cap=cap, nb=nb)
            fill(cache, k, v_, lens)
            O = split_attend(cache, q, lens)
        for b, (Q, K, V, L) in enumerate(seqs):
            ref = sr.attention_f64(Q, K, V, L, h, h_kv)
            err = float(np.abs(O[b] - ref).max())
            print(f"{label} sequence {b}: max|gpu - float64| = {err:.3e}")
            assert sr.within_bound(variant, O[b], ref), (label, b, err)
        ran += 1
    assert ran >= 4


# ---- 6. paged is contiguous ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk", sr.CHUNKS)
@pytest.mark.parametrize("page_rows", [64, 128])
@pytest.mark.parametrize("heads", HEADS, ids=HEAD_IDS)
@pytest.mark.parametrize("variant,d", BUILT)
def test_paged_is_contiguous(dev, variant, d, heads, page_rows, chunk):
    Q, K, V = dev_inputs(dev, d, heads)
    table = table_dev(dev, TABLES[page_rows])
    for lens, Nq in SHAPES[1::2]:
        cont, pool = new_cont(dev, variant, d, heads, chunk, cap=PCAP), new_pool(dev, variant, d, heads, page_rows, chunk)
        fill(cont, K, V, lens), fill(pool, K, V, lens, table)
        q = Q[:, :Nq].contiguous()
        cont.split_scratch.fill_(0xFF), pool.split_scratch.fill_(0xFF)
        want, got = split_attend(cont, q, lens), split_attend(pool, q, lens, table)
        assert_bits(f"paged against contiguous, lens {lens} Nq {Nq}", got, want)
        torch.cuda.synchronize()
        assert torch.equal(cont.split_scratch, pool.split_scratch), "the partials differ"


@pytest.mark.parametrize("variant,d", BUILT)
def test_two_sequences_share_a_prefix_page(dev, variant, d):
    """Sequences 0 and 1 name the same first page, written once through sequence 0; each continues in a page of its own."""
    Q, K, V = dev_inputs(dev, d, HEADS[0])
    page_rows, n, chunk = 64, 37, 64
    Kc, Vc = K.clone(), V.clone()
    Kc[1, :page_rows], Vc[1, :page_rows] = K[0, :page_rows], V[0, :page_rows]  # the contiguous cache holds the prefix twice
    table = table_dev(dev, TABLES[page_rows])
    table[1, 0] = table[0, 0]
    cont, pool = new_cont(dev, variant, d, HEADS[0], chunk, cap=PCAP), new_pool(dev, variant, d, HEADS[0], page_rows, chunk)
    lens = [page_rows + n] * B
    fill(cont, Kc, Vc, lens)
    fill(pool, Kc, Vc, [page_rows, 0, page_rows], table)  # the prefix, sequence 1 left out
    pos = i32(dev, [page_rows] * B)
    pool.append_paged(Kc[:, page_rows:page_rows + n].contiguous(), Vc[:, page_rows:page_rows + n].contiguous(), pos, table)
    for Nq in (1, 5):
        q = Q[:, :Nq].contiguous()
        assert_bits(f"shared prefix Nq {Nq}", split_attend(pool, q, lens, table), split_attend(cont, q, lens))
        for x, w in zip(partials(pool, Nq), partials(cont, Nq)):
            assert_bits("shared prefix: the partials", x[:, :2], w[:, :2])


# ---- 7. a decode loop under graph replay ------------------------------------------------------------------------------------
@pytest.mark.parametrize("paged", [False, True], ids=["contiguous", "paged"])
@pytest.mark.parametrize("variant,d", [(INT8, 64), (F16, 128)])
def test_decode_loop_under_graph_replay(dev, variant, d, paged):
    """One append (n = 1) and one split attend (Nq = 1) captured once on a side stream (single stream, linear) over static
    tensors; 35 replays, between which the new K, V, Q rows are copied in and pos / lens advance by 1 on that stream.
    Sequences 0 and 1 start at 40 and 110 rows: with chunks of 64 rows sequence 0 enters its second chunk, sequence 1 its
    third (and, paged, a new page, all of whose entries are in the table from the start).  Sequence 2 is an empty slot.
    Every replay equals the eager split call on a cache of its own."""
    chunk, page_rows = 64, 64
    Q, K, V = dev_inputs(dev, d, HEADS[0])
    start, steps = [40, 110], 35
    table = table_dev(dev, TABLES[page_rows]) if paged else None
    make = (lambda: new_pool(dev, variant, d, HEADS[0], page_rows, chunk)) if paged else (lambda: new_cont(dev, variant, d, HEADS[0], chunk, cap=PCAP))
    cache, yard = make(), make()
    fill(cache, K, V, start + [0], table), fill(yard, K, V, start + [0], table)
    append = (lambda c, k, v, p: c.append_paged(k, v, p, table)) if paged else (lambda c, k, v, p: c.append_tokens(k, v, p))
    attend = (lambda c, q, ln, out: c.attend_paged_split(q, ln, table, out=out)) if paged else (lambda c, q, ln, out: c.attend_tokens_split(q, ln, out=out))
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
        attend(cache, qs, lens, buf[:qs.numel()])
        pos.copy_(i32(dev, start + [-1]))
        lens.copy_(i32(dev, [L + 1 for L in start] + [0]))
        inc = i32(dev, [1, 1, 0])
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            append(cache, ks, vs, pos)
            attend(cache, qs, lens, buf[:qs.numel()])
        for k in range(steps):
            rows = [L + k for L in start] + [0]
            qs.copy_(qrow(k)), ks.copy_(row(K, rows)), vs.copy_(row(V, rows))
            graph.replay()
            got.append(buf.clone())
            pos.add_(inc), lens.add_(inc)
        side.synchronize()
    torch.cuda.current_stream(dev).wait_stream(side)
    assert pos.tolist() == [40 + steps, 110 + steps, -1]
    assert all(L // chunk != (L + steps) // chunk for L in start)  # both sequences end in another chunk than they began in
    for k, g in enumerate(got):  # the eager path, step by step
        rows = [L + k for L in start] + [-1]
        append(yard, row(K, rows), row(V, rows), i32(dev, rows))
        gd = Guarded(qs)
        attend(yard, qrow(k), i32(dev, [L + k + 1 for L in start] + [0]), gd.buf[:gd.n])
        want = gd.result()
        g = g.cpu().numpy()
        assert (g[qs.numel():] == GUARD).all(), "O written past its last row"
        o = g[:qs.numel()].reshape(qs.shape)
        assert_bits(f"replay {k}", o[:2], want[:2])
        assert np.abs(o[:2]).max() > 0.0
        assert_zeros(f"replay {k}: the empty slot", o[2])


# ---- 8. both bindings ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("heads", [HEADS[0], HEADS[1]], ids=HEAD_IDS[:2])
@pytest.mark.parametrize("variant,d", [(INT8, 64), (F16, 64)])
def test_compiled_binding_gives_the_same_bytes(dev, variant, d, heads):
    Q, K, V = dev_inputs(dev, d, heads)
    q = Q[:, :5].contiguous()
    lens = [45, 171, 0]
    table = table_dev(dev, TABLES[64])
    for paged in (False, True):
        outs, scratches = [], []
        for mod in (None, compiled_module()):
            c = new_pool(dev, variant, d, heads, 64, 64, mod=mod) if paged else new_cont(dev, variant, d, heads, 64, mod=mod)
            fill(c, K, V, lens, table if paged else None)
            outs.append(split_attend(c, q, lens, table if paged else None))
            plain = c.attend_paged_split(q, i32(dev, lens), table) if paged else c.attend_tokens_split(q, i32(dev, lens))
            torch.cuda.synchronize()
            assert plain.shape == q.shape and np.array_equal(plain.cpu().numpy(), outs[-1])
            parts = c.split_partials(5)
            nc = -(-(PCAP if paged else CAP) // 64)
            assert [tuple(x.shape) for x in parts] == [(B, nc, 5, q.shape[2]), (B, nc, 5, heads[0]), (B, nc, 5, heads[0])]
            scratches.append(c.split_scratch.clone())
        assert_bits("compiled against ctypes", outs[1], outs[0])
        assert torch.equal(scratches[0], scratches[1])
        assert_zeros("the empty slot", outs[0][2])
        assert np.abs(outs[0][:2]).max() > 0.0
    for mod in (None, compiled_module()):  # the refusals
        c = gs.new_cache(dev, variant, B, CAP, d, *heads, mod=mod)
        with pytest.raises(RuntimeError, match="enable_split"):
            c.attend_tokens_split(q, i32(dev, lens))
        for bad in (0, 32, 96, CAP + 32):
            with pytest.raises(RuntimeError, match="multiple of 64"):
                c.enable_split(bad)
        c.enable_split(64, 4)
        with pytest.raises(RuntimeError, match="max_nq"):
            c.attend_tokens_split(q, i32(dev, lens))
        with pytest.raises(RuntimeError, match="int32"):
            c.attend_tokens_split(q[:, :1].contiguous(), i32(dev, lens).to(torch.int64))
        al = lambda x: -(-x // 256) * 256  # noqa: E731 -- B sequences, 4 chunks, 4 rows
        assert c.split_scratch.numel() == al(4 * B * 4 * 4 * q.shape[2]) + 2 * al(4 * B * 4 * 4 * heads[0])


# ---- 9. one chunk ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("heads", [HEADS[0], HEADS[1]], ids=HEAD_IDS[:2])
@pytest.mark.parametrize("variant,d", BUILT)
def test_one_chunk_is_attend_tokens_within_the_combine_rounding(dev, variant, d, heads):
    """chunk_rows >= ceil64(L): one chunk, whose partial is attend_tokens' O bit for bit (the same tiles from the same zero
    state).  The combine then forms a_0 = l_0 2^0 = l_0 exactly, Ltot = l_0, rnd(l_0 Oc) and rnd(rnd(l_0 Oc) / l_0): two
    roundings of half an ulp each, so O is attend_tokens' O within one ulp and not bit-equal in general ((x l) / l is x only
    when the product is exact).  Asserted: Oc's bits, and |O - attend_tokens| <= 6 x 2^-23 |Oc|, the combine bound at n_c = 1."""
    Q, K, V = dev_inputs(dev, d, heads)
    for cap, chunk, lens, Nq in ((CAP, 128, [33, 95, 128], 5), (CAP, 192, [1, 160, 192], 1), (PCAP, PCAP, [40, 100, 224], 40)):
        cache = new_cont(dev, variant, d, heads, chunk, cap=cap)
        fill(cache, K, V, lens)
        q = Q[:, :Nq].contiguous()
        g = Guarded(q)
        cache.attend_tokens(q, i32(dev, lens), out=g.buf[:g.n])
        want = g.result()
        got = split_attend(cache, q, lens)
        Oc = partials(cache, Nq)[0]
        assert_bits(f"one chunk of {chunk} rows, lens {lens}: the partial", Oc[:, 0], want)
        err = np.abs(got.astype(np.float64) - want)
        print(f"chunk {chunk} lens {lens} Nq {Nq}: {int((got != want).sum())} of {got.size} elements differ, worst "
              f"{float((err / np.maximum(np.abs(want), 1e-30)).max() * 2 ** 23):.2f} x 2^-23 relative")
        assert (err <= 6 * 2.0 ** -23 * np.abs(want)).all(), (chunk, lens, float(err.max()))
