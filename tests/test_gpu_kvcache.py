"""GPU tests (MI355X) of the persistent K/V cache: qmha_kv_cache_append / qmha_attend_cached through
torch_ext.KVCache (ctypes) and the compiled module's class.

The oracle is the shipped path, so no arithmetic is restated here:
  * attend() after appends totalling `len` rows equals flash_solve_rect(Q, K[:, :len], V[:, :len], causal) BIT FOR BIT
    whenever that call takes its rectangular kernel (Nq != len, or no mask): both run the same Rect instance on
    byte-equal operands over the same tiles in the same order.
  * at len == Nq with the mask, qmha_solve_rect takes the SquareCausal instance while the cache runs Rect with
    diag_off = 0, so the result is held to the variant's bound against tests/causal_ref.py -- int8: every element
    within 2 u_r + 5e-5 of the base-2 restatement (all rows, the first 32 included: the restatement carries V's
    quantisation step, so DESIGN.md 10.1's 1.5-step allowance against float64 is not needed); fp16: fp16_lazy_tol --
    and whether it was also bit-identical is printed.
  * the cache's bytes equal what the pre-pass of a whole call writes: int8 K rows and scales against
    qmha_quantize_int8, fp16 K against a host half(), and the whole cache tensor (V operand blocks and scales
    included, and every byte no append should touch) against a second cache filled by ONE append.
Every attend writes O into a buffer with a sentinel-filled guard behind it, which must come back untouched.
Shapes: at most 512 rows, B = 2 (the chunk's and the cache's batch strides differ), H = 2.
"""
import ctypes
import functools
import threading

import numpy as np
import pytest

from tests import causal_ref as cr
from tests import gpu_support as gs
from tests import rect_ref as rr
from tests.gpu_support import (BUILT, CAUSAL, F16, INT8, assert_bits, assert_f16, assert_int8, attend, c_solve,  # noqa: F401
                               cache_array, compiled_module, dev, to_dev)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
B, H = 2, 2
TAG = "+kv"  # this file's mark on its parity_log records


def new_cache(dev, variant, d, cap, batch=B):
    return gs.new_cache(dev, variant, batch, cap, d, H)


def rect(variant, d, Q, K, V, causal=True):
    """The oracle: the shipped qmha_solve_rect on the same device tensors."""
    from quantizedmha_amd import torch_ext
    out = torch_ext.flash_solve_rect(Q, K.contiguous(), V.contiguous(), H * d, H, variant, causal=causal)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def assert_square_causal(label, variant, d, got, Q, K, V, oracle_rect=None):
    """len == Nq with the mask: the variant's bound against tests/causal_ref.py on host arrays Q, K, V [B, N, H d];
    oracle_rect (the SquareCausal instance's result) only for the record."""
    from oracle import oracle
    N = Q.shape[1]
    if variant == INT8:
        ref, unit, _ = cr.fa_int8(oracle, Q, K, V, H * d, H, causal=True, base2=True)
        assert_int8(label, got, ref, cr.per_element(unit, d), TAG)
    else:
        assert_f16(label, got, cr.fa_fp16_lazy(None, Q, K, V, H * d, H, causal=True)[0], cr.fp16_lazy_tol(N), TAG)
    if oracle_rect is not None:
        same = np.array_equal(got, oracle_rect)
        print(f"{label}: Rect with diag_off = 0 {'is' if same else 'is NOT'} bit-identical to the SquareCausal instance"
              f" (max difference {np.abs(got - oracle_rect).max():.3e})")


# ---- 1. the cache's bytes ------------------------------------------------------------------------------------
def carve(cache, d):
    """Views of the cache tensor by the workspace carve at N = cap: (K rows [B*H, cap, d], K scales or None)."""
    if cache.kernel == INT8:
        return cache_array(cache, "Ki", torch.int8).view(B * H, cache.cap, d), cache_array(cache, "sK", torch.float32)
    return cache_array(cache, "Kh", torch.float16).view(B * H, cache.cap, d), None


@pytest.mark.parametrize("variant,d", BUILT)
def test_cache_bytes_are_the_prepass_bytes(dev, variant, d):
    from quantizedmha_amd import torch_ext
    cap, C = 256, 64
    _, K, V = to_dev(dev, *cr.inputs(cap, H * d, B, "normal", 700 + d))
    cache = new_cache(dev, variant, d, cap)
    for c in range(cap // C):
        n = C * (c + 1)
        cache.append(K[:, n - C:n], V[:, n - C:n])
        assert cache.len == n
        torch.cuda.synchronize()
        rows, scales = carve(cache, d)
        if variant == INT8:
            Xi, sc = torch_ext.quantize_int8(K[:, :n].contiguous(), H * d, H, layout=0)
            torch.cuda.synchronize()
            assert torch.equal(rows[:, :n], Xi.view(B * H, n, d)), (n, "Ki")
            assert torch.equal(scales[:, :n // 32].view(torch.int32), sc.view(B * H, n // 32).view(torch.int32)), (n, "sK")
        else:
            want = K[:, :n].cpu().reshape(B, n, H, d).permute(0, 2, 1, 3).half().contiguous().view(B * H, n, d)
            assert torch.equal(rows[:, :n].cpu().view(torch.int16), want.view(torch.int16)), (n, "Kh")
        once = new_cache(dev, variant, d, cap)  # one append of n rows: the same bytes everywhere, V and its scales included
        once.append(K[:, :n], V[:, :n])
        torch.cuda.synchronize()
        assert torch.equal(cache.mem, once.mem), (n, "one append against many")


# ---- 2. chunked prefill ----------------------------------------------------------------------------------------
def chunked_prefill(dev, variant, d, t, cap=256, C=64, stream=None, cls=None):
    """Chunks of C rows: append, then attend with the chunk's queries; the list of O chunks (numpy)."""
    Q, K, V = t
    with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(dev)):
        cache = cls(B, cap, H * d, H, variant, str(dev)) if cls is not None else new_cache(dev, variant, d, cap)
        outs = []
        for c in range(cap // C):
            n = C * (c + 1)
            cache.append(K[:, n - C:n], V[:, n - C:n])
            outs.append(cache.attend(Q[:, n - C:n].contiguous(), causal=True))
        torch.cuda.current_stream(dev).synchronize()
    return [o.cpu().numpy() for o in outs]


@functools.lru_cache(maxsize=None)
def prefill_inputs(d, dist):
    return cr.inputs(256, H * d, B, dist, 710 + d)


@pytest.mark.parametrize("dist", rr.DISTS)
@pytest.mark.parametrize("variant,d", BUILT)
def test_chunked_prefill(dev, variant, d, dist):
    from oracle import oracle
    N, C = 256, 64
    Q, K, V = prefill_inputs(d, dist)
    t = to_dev(dev, Q, K, V)
    cache = new_cache(dev, variant, d, N)
    parts = []
    for c in range(N // C):
        n = C * (c + 1)
        cache.append(t[1][:, n - C:n], t[2][:, n - C:n])
        q = t[0][:, n - C:n].contiguous()
        got = attend(cache, q)
        want = rect(variant, d, q, t[1][:, :n], t[2][:, :n])
        if c == 0:  # len == Nq: the SquareCausal instance on the rect side
            assert_square_causal(f"kv prefill chunk 1 {variant} d{d} {dist}", variant, d, got, Q[:, :C], K[:, :C], V[:, :C], want)
        else:
            assert_bits(f"chunk {c + 1}", got, want)
        parts.append(got)
    got = np.concatenate(parts, axis=1)
    square = c_solve("opts", variant, t, H, CAUSAL)
    label = f"kv prefill {variant} d{d} {dist}"
    if variant == INT8:
        ref, unit, _ = cr.fa_int8(oracle, Q, K, V, H * d, H, causal=True, base2=True)
        pe = cr.per_element(unit, d)
        assert_int8(label, got, ref, pe, TAG)
        assert_int8(label + " (vs the square GPU call)", got, square.astype(np.float64), pe, TAG)
    else:
        assert_f16(label, got, cr.fa_fp16_lazy(None, Q, K, V, H * d, H, causal=True)[0], cr.fp16_lazy_tol(N), TAG)
        assert_f16(label + " (vs the square GPU call)", got, square, cr.fp16_lazy_tol(N), TAG)
        assert oracle.verify_results(got, cr.attention_f64(Q, K, V, H * d, H, causal=True).astype(np.float32), 1e-3, 1e-3) == -1


# ---- 3. uneven appends, odd tile count ---------------------------------------------------------------------------
@pytest.mark.parametrize("dist", rr.DISTS)
@pytest.mark.parametrize("variant,d", BUILT)
def test_uneven_appends_and_partial_last_stage(dev, variant, d, dist):
    """cap = 224: Gk = 7, the last stage is partial.  Appends of 32, 96, 32, 64 rows; decode-like Nq = 32 at len = 160
    (one active wave, offset 4), Nq = 160 at len = 160 (diag_off = 0, nqb = 2), Nq = 96 at len = cap."""
    cap = 224
    Q, K, V = rr.inputs(160, cap, H * d, B, dist, 720 + d)
    t = to_dev(dev, Q, K, V)
    cache = new_cache(dev, variant, d, cap)
    at = 0
    for n in (32, 96, 32):
        cache.append(t[1][:, at:at + n], t[2][:, at:at + n])
        at += n
    assert cache.len == 160
    q = t[0][:, :32].contiguous()
    assert_bits("Nq 32 at len 160", attend(cache, q), rect(variant, d, q, t[1][:, :160], t[2][:, :160]))
    got = attend(cache, t[0])
    assert_square_causal(f"kv Nq 160 at len 160 {variant} d{d} {dist}", variant, d, got, Q, K[:, :160], V[:, :160],
                         rect(variant, d, t[0], t[1][:, :160], t[2][:, :160]))
    cache.append(t[1][:, 160:], t[2][:, 160:])
    assert cache.len == cap
    q = t[0][:, 32:128].contiguous()
    assert_bits("Nq 96 at len 224", attend(cache, q), rect(variant, d, q, t[1], t[2]))


# ---- 4. len far below cap ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dist", rr.DISTS)
@pytest.mark.parametrize("variant,d", BUILT)
def test_short_length_in_a_large_cache(dev, variant, d, dist):
    """cap = 512, len = 64: almost every tile of a slice lies beyond the valid rows."""
    Q, K, V = rr.inputs(64, 64, H * d, B, dist, 730 + d)
    t = to_dev(dev, Q, K, V)
    cache = new_cache(dev, variant, d, 512)
    cache.append(t[1], t[2])
    assert_square_causal(f"kv Nq 64 at len 64 of 512 {variant} d{d} {dist}", variant, d, attend(cache, t[0]), Q, K, V,
                         rect(variant, d, t[0], t[1], t[2]))
    q = t[0][:, 32:].contiguous()
    assert_bits("Nq 32 at len 64 of 512", attend(cache, q), rect(variant, d, q, t[1], t[2]))


# ---- 5. a stale tail -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant,d", BUILT)
def test_stale_tail_is_never_read(dev, variant, d):
    """A cache filled to cap with rows of magnitude 1e30 (inf in Kh, huge sK / sV), truncated to 64 and refilled with
    64 real rows, attends at len = 128 exactly as a fresh zero-filled cache does."""
    cap = 256
    Q, K, V = rr.inputs(64, 128, H * d, B, "normal", 740 + d)
    t = to_dev(dev, Q, K, V)
    huge = torch.full((B, cap, H * d), 1e30, dtype=torch.float32, device=dev)
    huge[:, :64] = t[1][:, :64]
    hugev = torch.full((B, cap, H * d), -1e30, dtype=torch.float32, device=dev)
    hugev[:, :64] = t[2][:, :64]
    stale = new_cache(dev, variant, d, cap)
    stale.append(huge, hugev)
    stale.truncate(64)
    assert stale.len == 64
    stale.append(t[1][:, 64:], t[2][:, 64:])
    fresh = new_cache(dev, variant, d, cap)
    fresh.append(t[1][:, :64], t[2][:, :64])
    fresh.append(t[1][:, 64:], t[2][:, 64:])
    got = attend(stale, t[0])
    assert np.isfinite(got).all()
    assert_bits("stale tail", got, attend(fresh, t[0]))
    assert_bits("stale tail against the rect call", got, rect(variant, d, t[0], t[1], t[2]))


# ---- 6. no mask, a full cache -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dist", rr.DISTS)
@pytest.mark.parametrize("cap,Nq", [(96, 160), (256, 64)])
@pytest.mark.parametrize("variant,d", BUILT)
def test_non_causal_over_a_full_cache(dev, variant, d, cap, Nq, dist):
    from quantizedmha_amd import _lib
    t = to_dev(dev, *rr.inputs(Nq, cap, H * d, B, dist, 750 + d + cap))
    cache = new_cache(dev, variant, d, cap)
    cache.append(t[1][:, :32], t[2][:, :32])
    with pytest.raises(_lib.QMHAError, match="no unmasked mode"):
        cache.attend(t[0], causal=False)
    cache.append(t[1][:, 32:], t[2][:, 32:])
    assert_bits("non-causal", attend(cache, t[0], causal=False), rect(variant, d, t[0], t[1], t[2], causal=False))


# ---- 7. hard numerics -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant,d", [(INT8, 64), (F16, 64)])
def test_spike_tile_through_the_cache(dev, variant, d):
    """`spike_tile` (160, 256) causal (B = 1), built by appending 96 + 160 rows: the int8 re-anchor and the fp16
    rebase on a tile that some waves of a workgroup skip."""
    t = to_dev(dev, *rr.hard_inputs("spike_tile", d, 160, 256))
    cache = new_cache(dev, variant, d, 256, batch=1)
    cache.append(t[1][:, :96], t[2][:, :96])
    cache.append(t[1][:, 96:], t[2][:, 96:])
    got = attend(cache, t[0])
    assert np.isfinite(got).all()
    assert_bits("spike_tile", got, rect(variant, d, t[0], t[1], t[2]))


# ---- 8. profile records ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant,d", [(INT8, 64), (F16, 64)])
def test_profile_records_append_and_attend(dev, variant, d):
    from quantizedmha_amd import _lib
    lib = _lib.load()
    t = to_dev(dev, *rr.inputs(64, 128, H * d, B, "normal", 760))
    cache = new_cache(dev, variant, d, 128)
    lib.qmha_profile_collect(None, None, None)
    lib.qmha_profile_enable(1)
    try:
        cache.append(t[1], t[2])
        cache.attend(t[0])
        main_ms, pre_ms, calls = ctypes.c_double(), ctypes.c_double(), ctypes.c_longlong()
        assert lib.qmha_profile_collect(ctypes.byref(main_ms), ctypes.byref(calls), ctypes.byref(pre_ms)) == 0
    finally:
        lib.qmha_profile_enable(0)
    assert calls.value == 2 and main_ms.value > 0.0 and pre_ms.value > 0.0, (calls.value, main_ms.value, pre_ms.value)


# ---- 9. two host threads --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant,d", BUILT)
def test_two_threads_with_their_own_caches(dev, variant, d):
    t = to_dev(dev, *prefill_inputs(d, "normal"))
    want = chunked_prefill(dev, variant, d, t)
    streams = [torch.cuda.Stream(device=dev) for _ in range(2)]
    for s in streams:
        s.wait_stream(torch.cuda.current_stream(dev))
    results, errors = [None, None], []

    def work(i):
        try:
            results[i] = chunked_prefill(dev, variant, d, t, stream=streams[i])
        except Exception as e:  # noqa: BLE001 -- reported by the assertion below
            errors.append(e)

    threads = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    torch.cuda.synchronize()
    assert not errors, errors
    for got in results:
        assert len(got) == len(want) and all(np.array_equal(g, w) for g, w in zip(got, want))


# ---- 10. both bindings --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant,d", BUILT)
def test_compiled_binding_gives_the_same_bytes(dev, variant, d):
    compiled = compiled_module()
    t = to_dev(dev, *prefill_inputs(d, "normal"))
    want = chunked_prefill(dev, variant, d, t)
    got = chunked_prefill(dev, variant, d, t, cls=compiled.KVCache)
    assert np.array_equal(got[-1], want[-1]) and all(np.array_equal(g, w) for g, w in zip(got, want))
    c = compiled.KVCache(1, 64, H * d, H, variant)  # B = 1 takes [n, d_model]
    c.append(t[1][0, :64], t[2][0, :64])
    assert c.len == 64 and c.cap == 64
    one = c.attend(t[0][0, 32:64].contiguous())
    torch.cuda.synchronize()
    assert one.shape == (32, H * d)
    assert_bits("B = 1", one.cpu().numpy(), rect(variant, d, t[0][:1, 32:64].contiguous(), t[1][:1, :64], t[2][:1, :64])[0])
    c.truncate(32)
    assert c.len == 32
    with pytest.raises(RuntimeError, match="exceed cap"):
        c.append(t[1][0, :64], t[2][0, :64])
