"""GPU tests (MI355X) of grouped-query attention: qmha_solve_gqa and qmha_kv_cache_create_gqa through
the ctypes binding (flash_solve_gqa, GroupedKVCache) and the compiled module.

The oracle is the shipped multi-head path, so no arithmetic is restated for the shape tests: a multi-head KVCache over
K and V expanded G = h / h_kv times along the head axis.  The cached attend always runs the Rect instance (square and
unmasked shapes included), a query head's grouped sweep visits the same tiles in the same order on byte-equal
operands, so EVERY comparison against it is bit for bit: a wrong slice index, unit split, stride or diag_off moves
whole tiles.  So that the suite does not rest on two GPU paths agreeing alone, one test per variant also holds a
grouped result to tests/rect_ref.py on the expanded inputs at the rectangular tests' bounds (int8: 2 u_r + 5e-5 of the
base-2 restatement; fp16: fp16_lazy_tol(Nk) of the lazy contract and max(1e-3, 1e-3 |ref|) of float64).
Every O is the head of a buffer with a sentinel-filled guard behind it.  Shapes: at most 256 rows; B = 2 and h_kv = 2
unless stated, so that b > 0 and kvh > 0 occur in the K/V slice index.
"""
import ctypes
import functools

import numpy as np
import pytest

from tests import causal_ref as cr
from tests import rect_ref as rr
from tests.gpu_support import (BUILT, CAUSAL, F16, GUARD, INT8, assert_bits, attend, c_solve, cache_array,  # noqa: F401
                               compiled_module, dev, overlap_chunks, to_dev)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
B, HKV = 2, 2


@functools.lru_cache(maxsize=None)
def host_inputs(Nq, Nk, d, h, h_kv, batch, dist, seed):
    """Q [batch, Nq, h d], K and V [batch, Nk, h_kv d] (rect_ref.inputs' distributions)."""
    Q, K, V = rr.inputs(Nq, Nk, h * d, batch, dist, seed)
    return Q, np.ascontiguousarray(K[..., :h_kv * d]), np.ascontiguousarray(V[..., :h_kv * d])


def expand(X, h_kv, G):
    """[B, N, h_kv d] -> [B, N, h_kv G d]: K/V head kvh repeated for query heads kvh G .. kvh G + G - 1."""
    b, n, w = X.shape
    d = w // h_kv
    if isinstance(X, np.ndarray):
        return np.ascontiguousarray(np.repeat(X.reshape(b, n, h_kv, d), G, axis=2).reshape(b, n, h_kv * G * d))
    return X.view(b, n, h_kv, d).repeat_interleave(G, dim=2).reshape(b, n, h_kv * G * d).contiguous()


def solve_gqa(variant, t, d, h, h_kv, flags, **kw):
    """qmha_solve_gqa on device tensors t = [Q [B, Nq, h d], K, V [B, Nk, h_kv d]]; O (numpy) through the guard."""
    assert t[1].shape[2] == h_kv * d and t[0].shape[2] == h * d
    return c_solve("gqa", variant, t, h, flags, h_kv=h_kv, **kw)


def grouped_cached(dev, variant, d, h, h_kv, t, causal, cap=None, stale=False, cls=None):
    """The grouped cache: K and V appended in two pieces (one if 32 rows), then attend.  stale: the cache is first
    filled to cap with rows of magnitude 1e30 and truncated to 0, so whatever lies beyond len is poison."""
    from quantizedmha_amd import torch_ext
    Q, K, V = t
    n = K.shape[1]
    cap = n if cap is None else cap
    cache = (cls or torch_ext.GroupedKVCache)(Q.shape[0], cap, h * d, h, h_kv, variant, str(dev))
    if stale:
        cache.append(torch.full((Q.shape[0], cap, h_kv * d), 1e30, dtype=torch.float32, device=dev),
                     torch.full((Q.shape[0], cap, h_kv * d), -1e30, dtype=torch.float32, device=dev))
        cache.truncate(0)
    cut = (n // 64) * 32
    if cut:
        cache.append(K[:, :cut], V[:, :cut])
    cache.append(K[:, cut:], V[:, cut:])
    assert cache.len == n
    if cls is not None:
        out = cache.attend(Q, causal=causal)
        torch.cuda.synchronize()
        return out.cpu().numpy()
    return attend(cache, Q, causal)


def oracle_cached(dev, variant, d, h, h_kv, t, causal, cap=None):
    """The oracle: the shipped multi-head KVCache over K and V expanded to h heads (always the Rect instance)."""
    from quantizedmha_amd import torch_ext
    Q, K, V = t
    cap = K.shape[1] if cap is None else cap
    cache = torch_ext.KVCache(Q.shape[0], cap, h * d, h, variant, device=dev)
    cache.append(expand(K, h_kv, h // h_kv), expand(V, h_kv, h // h_kv))
    return attend(cache, Q, causal)


# ---- 1. shapes: every comparison bit for bit against the expanded multi-head cache -------------------------------
# (G, Nq, Nk, causal, head sizes or None = every built one): what each reaches is in DESIGN.md 14.4
SHAPES = [
    (2, 96, 160, True, None),    # U = 6: a workgroup mixes two query groups; second workgroup half active; int8 nqb = 2
    (4, 96, 96, True, None),     # square: nqb = 3, unpaired middle block; diag_off = 0
    (3, 64, 96, True, None),     # non-power-of-two u / G
    (3, 64, 96, False, None),
    (8, 32, 96, True, (32, 64)),  # two workgroups per query group
    (2, 160, 96, False, None),   # Nq > Nk without the mask
    (2, 128, 128, False, None),  # square and unmasked: the grouped kernel all the same
]


def shape_id(s):
    return f"G{s[0]}-Nq{s[1]}-Nk{s[2]}-{'causal' if s[3] else 'full'}"


SHAPE_RUNS = [pytest.param(s, v, d, id=f"{shape_id(s)}-{v}-d{d}") for s in SHAPES for v, d in BUILT if s[4] is None or d in s[4]]


@pytest.mark.parametrize("dist", rr.DISTS)
@pytest.mark.parametrize("shape,variant,d", SHAPE_RUNS)
def test_grouped_equals_expanded_multi_head(dev, shape, variant, d, dist):
    G, Nq, Nk, causal, _ = shape
    h = HKV * G
    t = to_dev(dev, *host_inputs(Nq, Nk, d, h, HKV, B, dist, 800 + Nq + Nk + G))
    want = oracle_cached(dev, variant, d, h, HKV, t, causal)
    assert_bits("solve_gqa", solve_gqa(variant, t, d, h, HKV, CAUSAL if causal else 0), want)
    assert_bits("grouped cache", grouped_cached(dev, variant, d, h, HKV, t, causal), want)


@pytest.mark.parametrize("variant,d", BUILT)
def test_square_unmasked_equals_the_rect_call_on_query_halves(dev, variant, d):
    """Nq = Nk = 128 without the mask: the expanded qmha_solve_rect with Q in two halves of 64 rows (Nq != Nk, so its
    rectangular kernel)."""
    from quantizedmha_amd import torch_ext
    G, N = 2, 128
    h = HKV * G
    t = to_dev(dev, *host_inputs(N, N, d, h, HKV, B, "normal", 810))
    Kx, Vx = expand(t[1], HKV, G), expand(t[2], HKV, G)
    halves = [torch_ext.flash_solve_rect(t[0][:, r:r + 64].contiguous(), Kx, Vx, h * d, h, variant) for r in (0, 64)]
    torch.cuda.synchronize()
    assert_bits("halves", solve_gqa(variant, t, d, h, HKV, 0), torch.cat(halves, dim=1).cpu().numpy())


@pytest.mark.parametrize("dist", rr.DISTS)
@pytest.mark.parametrize("variant,d", BUILT)
def test_decode_step_through_a_stale_cache(dev, variant, d, dist):
    """G = 4 (h = 8), Nq = 32 at len = 224 in cap = 256: four heads in one workgroup, Gk = 7 with a partial last
    stage, and a tail beyond len that holds 1e30 (inf in Kh, huge sK / sV) and is never read."""
    G, cap, n = 4, 256, 224
    h = HKV * G
    t = to_dev(dev, *host_inputs(32, n, d, h, HKV, B, dist, 820))
    want = oracle_cached(dev, variant, d, h, HKV, t, True, cap=cap)
    got = grouped_cached(dev, variant, d, h, HKV, t, True, cap=cap, stale=True)
    assert np.isfinite(got).all()
    assert_bits("decode", got, want)
    assert_bits("decode, own call", solve_gqa(variant, t, d, h, HKV, CAUSAL), want)


@pytest.mark.parametrize("variant,d", BUILT)
def test_spike_tile_in_the_grouped_instance(dev, variant, d):
    """rect_ref's `spike_tile` (160, 256) causal, its two K/V heads shared by G = 2 query heads each (both carry the
    hard problem's queries): the int8 re-anchor and the fp16 rebase inside the grouped instance."""
    G = 2
    Q, K, V = rr.hard_inputs("spike_tile", d, 160, 256)
    h_kv = cr.HARD["spike_tile"].h
    t = to_dev(dev, expand(Q, h_kv, G), K, V)
    want = oracle_cached(dev, variant, d, h_kv * G, h_kv, t, True)
    got = solve_gqa(variant, t, d, h_kv * G, h_kv, CAUSAL)
    assert np.isfinite(got).all()
    assert_bits("spike_tile", got, want)
    assert_bits("spike_tile, cache", grouped_cached(dev, variant, d, h_kv * G, h_kv, t, True), want)


# ---- 2. against the host restatements, at the rectangular tests' bounds ----------------------------------------------
REF_SHAPE = (2, 96, 160, 64)  # G, Nq, Nk, d


def test_int8_vs_base2_restatement_on_expanded_inputs(dev):
    from oracle import oracle
    G, Nq, Nk, d = REF_SHAPE
    h = HKV * G
    Q, K, V = host_inputs(Nq, Nk, d, h, HKV, B, "normal", 830)
    ref, unit = rr.fa_int8(oracle, Q, expand(K, HKV, G), expand(V, HKV, G), h * d, h, causal=True, base2=True)
    got = solve_gqa(INT8, to_dev(dev, Q, K, V), d, h, HKV, CAUSAL)
    assert np.isfinite(got).all()
    err = np.abs(got.astype(np.float64) - ref)
    pe = cr.per_element(unit, d)
    print(f"gqa int8: max|gpu - ref| = {err.max():.3e}, worst (err - 5e-5) / u_r = {cr.flip_units(err, pe):.3f} (bound 2)")
    assert (err <= 2.0 * pe + 5e-5).all(), (float(err.max()), cr.flip_units(err, pe))


def test_fp16_vs_lazy_contract_and_float64_on_expanded_inputs(dev):
    from oracle import oracle
    G, Nq, Nk, d = REF_SHAPE
    h = HKV * G
    Q, K, V = host_inputs(Nq, Nk, d, h, HKV, B, "normal", 830)
    Kx, Vx = expand(K, HKV, G), expand(V, HKV, G)
    contract = rr.fa_fp16_lazy(None, Q, Kx, Vx, h * d, h, causal=True)
    exact = rr.attention_f64(Q, Kx, Vx, h * d, h, True)
    got = solve_gqa(F16, to_dev(dev, Q, K, V), d, h, HKV, CAUSAL)
    assert np.isfinite(got).all()
    err = float(np.abs(got.astype(np.float64) - contract).max())
    print(f"gqa fp16: max|gpu - lazy contract| = {err:.3e} (bound {cr.fp16_lazy_tol(Nk):.2e}), "
          f"max|gpu - float64| = {float(np.abs(got - exact).max()):.3e}")
    assert err <= cr.fp16_lazy_tol(Nk), err
    assert oracle.verify_results(got, exact.astype(np.float32), 1e-3, 1e-3) == -1


# ---- 3. the grouped cache's bytes ---------------------------------------------------------------------------------
@pytest.mark.parametrize("variant,d", BUILT)
def test_grouped_cache_bytes_are_the_prepass_bytes_at_h_kv_heads(dev, variant, d):
    """After two appends: Ki / sK / sV against qmha_quantize_int8 with h = h_kv (fp16: Kh against a host half()), and
    the whole tensor -- Vh / Vt included -- against a multi-head cache of h_kv heads given the same rows."""
    from quantizedmha_amd import torch_ext
    G, cap, n = 2, 256, 160
    h = HKV * G
    _, K, V = to_dev(dev, *host_inputs(32, n, d, h, HKV, B, "normal", 840))
    cache = torch_ext.GroupedKVCache(B, cap, h * d, h, HKV, variant, device=dev)
    plain = torch_ext.KVCache(B, cap, HKV * d, HKV, variant, device=dev)
    for c in (cache, plain):
        c.append(K[:, :64], V[:, :64])
        c.append(K[:, 64:], V[:, 64:])
    torch.cuda.synchronize()
    assert cache.len == n and cache.mem.numel() == plain.mem.numel() > 1
    assert torch.equal(cache.mem, plain.mem)
    if variant == INT8:
        Ki = cache_array(cache, "Ki", torch.int8).view(B * HKV, cap, d)
        sK, sV = cache_array(cache, "sK", torch.int32), cache_array(cache, "sV", torch.int32)
        Xi, sc = torch_ext.quantize_int8(K, HKV * d, HKV, layout=0)
        _, scv = torch_ext.quantize_int8(V, HKV * d, HKV, layout=1)
        torch.cuda.synchronize()
        assert torch.equal(Ki[:, :n], Xi.view(B * HKV, n, d))
        assert torch.equal(sK[:, :n // 32], sc.view(B * HKV, n // 32).view(torch.int32))
        assert torch.equal(sV[:, :n // 32], scv.view(B * HKV, n // 32).view(torch.int32))
    else:
        Kh = cache_array(cache, "Kh", torch.int16).view(B * HKV, cap, d)
        want = K.cpu().reshape(B, n, HKV, d).permute(0, 2, 1, 3).half().contiguous().view(B * HKV, n, d)
        assert torch.equal(Kh[:, :n].cpu(), want.view(torch.int16))


# ---- 4. h_kv == h is the multi-head entry point ----------------------------------------------------------------------
@pytest.mark.parametrize("variant,Nq,Nk,flags", [("fa", 96, 96, 0), ("unfused", 96, 96, 0), ("fa_mfma", 96, 96, 0),
                                                 ("fa_tc_int8_pt", 96, 96, 0), (INT8, 96, 96, 0), (F16, 96, 96, 0),
                                                 (INT8, 96, 96, CAUSAL), (F16, 96, 96, CAUSAL),
                                                 (INT8, 96, 160, CAUSAL), (F16, 96, 160, 0)])
def test_equal_head_counts_are_qmha_solve_rect(dev, variant, Nq, Nk, flags):
    d, h = 64, 2
    t = to_dev(dev, *rr.inputs(Nq, Nk, h * d, B, "normal", 850))
    assert_bits("h_kv == h", solve_gqa(variant, t, d, h, h, flags), c_solve("rect", variant, t, h, flags))


@pytest.mark.parametrize("variant,d", BUILT)
def test_equal_head_counts_are_the_multi_head_cache(dev, variant, d):
    from quantizedmha_amd import torch_ext
    h = 2
    t = to_dev(dev, *rr.inputs(64, 160, h * d, B, "normal", 860))
    caches = [torch_ext.KVCache(B, 192, h * d, h, variant, device=dev),
              torch_ext.GroupedKVCache(B, 192, h * d, h, h, variant, device=dev),
              torch_ext.GroupedKVCache(B, 192, h * d, h, None, variant, device=dev)]
    outs = []
    for c in caches:
        c.append(t[1][:, :96], t[2][:, :96])
        c.append(t[1][:, 96:], t[2][:, 96:])
        outs.append(attend(c, t[0]))
    torch.cuda.synchronize()
    for c, o in zip(caches[1:], outs[1:]):
        assert torch.equal(c.mem, caches[0].mem)
        assert_bits("cache, h_kv == h", o, outs[0])


@pytest.mark.parametrize("variant", ["fa", "unfused", "fa_mfma", "fa_tc_int8_pt"])
def test_equal_head_counts_keep_the_cache_unbuilt_for_other_variants(dev, variant):
    from quantizedmha_amd import _lib, torch_ext
    with pytest.raises(_lib.QMHAError, match="K/V cache is not built"):
        torch_ext.GroupedKVCache(B, 64, 128, 2, 2, variant, device=dev)


# ---- 5. host layer ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [INT8, F16])
def test_overlap_chunks_are_bit_identical(dev, variant):
    G, d = 2, 64
    h = HKV * G
    t = to_dev(dev, *host_inputs(96, 160, d, h, HKV, 3, "normal", 870))
    want = solve_gqa(variant, t, d, h, HKV, CAUSAL)
    with overlap_chunks(2):
        got = solve_gqa(variant, t, d, h, HKV, CAUSAL)
    assert_bits("two chunks of B = 3", got, want)


@pytest.mark.parametrize("variant", [INT8, F16])
def test_caller_workspace_side_stream_and_profile_records(dev, variant):
    """Caller-owned scratch of exactly the stated size on a non-default stream equals the leased-slot result; one
    byte less is refused and leaves O alone; with profiling on, every call is one record with a pre-pass and a main
    time, and a grouped append and attend are one record each."""
    from quantizedmha_amd import _lib, torch_ext
    lib = _lib.load()
    G, d, Nq, Nk = 2, 64, 96, 160
    h = HKV * G
    t = to_dev(dev, *host_inputs(Nq, Nk, d, h, HKV, B, "uniform", 880))
    want = solve_gqa(variant, t, d, h, HKV, CAUSAL)
    need = lib.qmha_workspace_size(B, Nk, HKV * d, HKV, _lib.VARIANTS[variant])
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    assert_bits("caller workspace", solve_gqa(variant, t, d, h, HKV, CAUSAL, ws=ws, stream=s.cuda_stream), want)
    refused = solve_gqa(variant, t, d, h, HKV, CAUSAL, ws=ws, ws_bytes=need - 1, stream=s.cuda_stream, expect=1)
    assert (refused == GUARD).all()
    main_ms, pre_ms, calls = ctypes.c_double(), ctypes.c_double(), ctypes.c_longlong()
    lib.qmha_profile_collect(None, None, None)
    lib.qmha_profile_enable(1)
    try:
        for _ in range(3):
            assert_bits("profiled", solve_gqa(variant, t, d, h, HKV, CAUSAL), want)
        assert lib.qmha_profile_collect(ctypes.byref(main_ms), ctypes.byref(calls), ctypes.byref(pre_ms)) == 0
        assert calls.value == 3 and main_ms.value > 0.0 and pre_ms.value > 0.0, (calls.value, main_ms.value, pre_ms.value)
        cache = torch_ext.GroupedKVCache(B, Nk, h * d, h, HKV, variant, device=dev)
        cache.append(t[1], t[2])
        cache.attend(t[0])
        assert lib.qmha_profile_collect(ctypes.byref(main_ms), ctypes.byref(calls), ctypes.byref(pre_ms)) == 0
        assert calls.value == 2 and main_ms.value > 0.0 and pre_ms.value > 0.0, (calls.value, main_ms.value, pre_ms.value)
    finally:
        lib.qmha_profile_enable(0)


@pytest.mark.parametrize("variant", [INT8, F16])
@pytest.mark.parametrize("causal", [True, False])
def test_repeatable_and_batch_independent(dev, variant, causal):
    G, d = 2, 64
    h = HKV * G
    flags = CAUSAL if causal else 0
    t = to_dev(dev, *host_inputs(96, 160, d, h, HKV, B, "normal", 890))
    a = solve_gqa(variant, t, d, h, HKV, flags)
    assert_bits("again", solve_gqa(variant, t, d, h, HKV, flags), a)
    for b in range(B):
        one = solve_gqa(variant, [x[b:b + 1].contiguous() for x in t], d, h, HKV, flags)
        assert_bits(f"sequence {b} alone", one[0], a[b])


@pytest.mark.parametrize("variant", ["fa", "fa_tc_int8_pt", F16])
def test_unsupported_grouped_call_touches_nothing(dev, variant):
    from quantizedmha_amd import _lib
    d = 32 if variant == F16 else 64
    t = to_dev(dev, *host_inputs(64, 128, d, 4, 2, 1, "normal", 895))
    got = solve_gqa(variant, t, d, 4, 2, CAUSAL, expect=4)
    assert (got == GUARD).all()
    msg = _lib.load().qmha_last_error().decode()
    assert variant in msg and f"d = {d}" in msg and "grouped-query" in msg


# ---- 6. both bindings -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant,d", BUILT)
def test_bindings_give_the_same_bytes(dev, variant, d):
    from quantizedmha_amd import torch_ext
    compiled = compiled_module()
    G = 2
    h = HKV * G
    t = to_dev(dev, *host_inputs(96, 160, d, h, HKV, B, "normal", 900))
    for causal in (True, False):
        want = solve_gqa(variant, t, d, h, HKV, CAUSAL if causal else 0)
        out = torch.empty_like(t[0])
        got = torch_ext.flash_solve_gqa(t[0], t[1], t[2], h * d, h, HKV, variant, out=out, causal=causal)
        torch.cuda.synchronize()
        assert got is out
        assert_bits("ctypes", out.cpu().numpy(), want)
        got = compiled.flash_solve_gqa(t[0], t[1], t[2], h * d, h, HKV, variant, causal=causal)
        torch.cuda.synchronize()
        assert_bits("compiled", got.cpu().numpy(), want)
    want = grouped_cached(dev, variant, d, h, HKV, t, True)
    assert_bits("compiled cache", grouped_cached(dev, variant, d, h, HKV, t, True, cls=compiled.GroupedKVCache), want)
    one = torch_ext.flash_solve_gqa(t[0][0], t[1][0], t[2][0], h * d, h, HKV, variant, causal=True)  # [Nq, h d], [Nk, h_kv d]
    torch.cuda.synchronize()
    assert_bits("B = 1", one.cpu().numpy(), solve_gqa(variant, [x[:1].contiguous() for x in t], d, h, HKV, CAUSAL)[0])
    for mod in (torch_ext, compiled):
        with pytest.raises(RuntimeError, match="K and V must have the same shape"):
            mod.flash_solve_gqa(t[0], t[1], t[2][:, :128].contiguous(), h * d, h, HKV, variant)
        with pytest.raises(RuntimeError, match="h_kv"):
            mod.flash_solve_gqa(t[0], torch.zeros(B, 160, 3 * d, device=dev), torch.zeros(B, 160, 3 * d, device=dev), h * d,
                                h, 3, variant)  # 3 K/V heads under 4 query heads
    c = compiled.GroupedKVCache(B, 64, h * d, h, HKV, variant)
    with pytest.raises(RuntimeError, match="must be"):
        c.append(expand(t[1], HKV, G)[:, :32], expand(t[2], HKV, G)[:, :32])  # multi-head rows into a grouped cache
