"""What the GPU test files (tests/test_gpu_*.py) share: the variant constants, the `dev` fixture, the guarded output
buffer, the bounds the suites hold O to, the raw C-ABI call, the K/V cache helpers and the cache tensor's layout.

Importing this module needs neither a GPU nor torch (functions that use torch import it), so the CPU test files take
their constants from it too.  It is not collected, so pytest does not rewrite its asserts: each carries its message.
"""
import contextlib
import functools
import importlib.util
import os
import sysconfig

import numpy as np
import pytest

from tests import causal_ref as cr
from tests import parity_log

INT8, F16 = "fa_tc_int8_b", "fa_tc_v1a"
BUILT = [(INT8, 32), (INT8, 64), (INT8, 128), (F16, 64), (F16, 128)]  # every (variant, d) the masked kernels are built for
CAUSAL = 1  # QMHA_FLAG_CAUSAL
GUARD = 7.25  # the sentinel behind O (and in O, until a call writes it)


@pytest.fixture(scope="module")
def dev():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from quantizedmha_amd import _lib
    _lib.load()  # raises if the HIP library is missing: no silent fallback
    return torch.device("cuda:0")


def to_dev(dev, *xs):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in xs]


def i32(dev, xs):
    import torch
    return torch.tensor(xs, dtype=torch.int32, device=dev)


class Guarded:
    """O as the head of a buffer whose 32-row tail holds a sentinel that must survive the call; `out` (shaped like Q)
    or `buf[:n]` (flat) is what a call writes into.  The head starts as the sentinel too, so a refused call returns it."""

    def __init__(self, Q):
        import torch
        self.n, self.shape = Q.numel(), tuple(Q.shape)
        self.buf = torch.full((self.n + 32 * Q.shape[-1],), GUARD, dtype=torch.float32, device=Q.device)
        self.out = self.buf[:self.n].view(self.shape)
        torch.cuda.synchronize()  # the fill is done before a call on another stream may write O

    def device_result(self):
        import torch
        torch.cuda.synchronize()
        assert bool((self.buf[self.n:] == GUARD).all()), "O written past its last row"
        return self.out

    def result(self):
        return self.device_result().cpu().numpy()


# ---- the bounds ------------------------------------------------------------------------------------------------------
def assert_bits(label, got, want):
    assert np.isfinite(want).all(), (label, "the reference is not finite")
    assert np.array_equal(got, want), (label, float(np.abs(got - want).max()), int((got != want).sum()))


def assert_zeros(label, got):
    assert (got == 0.0).all() and not np.signbit(got).any(), (label, "not all positive zeros")


def assert_int8(label, got, ref, unit, tag):
    """Every element finite and within 2 u_r + 5e-5 of ref (u_r: the row's one-flip unit per element,
    tests/causal_ref.py); recorded in tests/parity_log.py under INT8 + tag."""
    assert np.isfinite(got).all(), (label, "O is not finite")
    err = np.abs(got.astype(np.float64) - ref)
    units = cr.flip_units(err, unit)
    frac = float((err > 5e-5).mean())
    parity_log.record(f"{label} [max error beyond 5e-5, in one-flip units]", INT8 + tag, units, frac, 2.0)
    print(f"{label}: max|gpu - ref| = {err.max():.3e}, worst (err - 5e-5) / u_r = {units:.3f} (bound 2), "
          f"frac > 5e-5 = {frac:.2e}, largest u_r = {float(np.max(unit)):.2e}")
    assert (err <= 2.0 * unit + 5e-5).all(), (label, float(err.max()), units)


def assert_f16(label, got, contract, tol, tag, exact=None, got_all=None):
    """Finite and within tol of the lazy contract; with `exact`, got_all (default got) also within
    max(1e-3, 1e-3 |ref|) of float64.  Recorded in tests/parity_log.py under F16 + tag."""
    assert np.isfinite(got).all(), (label, "O is not finite")
    err = float(np.abs(got.astype(np.float64) - contract).max())
    parity_log.record(f"{label} (vs lazy contract)", F16 + tag, err, float((np.abs(got - contract) > 5e-5).mean()), tol)
    print(f"{label}: max|gpu - lazy contract| = {err:.3e} (bound {tol:.2e})")
    assert err <= tol, (label, err, tol)
    if exact is not None:
        from oracle import oracle
        got_all = got if got_all is None else got_all
        far = float(np.abs(got_all - exact).max())
        parity_log.record(f"{label} (vs float64)", F16 + tag, far, float((np.abs(got_all - exact) > 5e-5).mean()), 1e-3)
        print(f"{label}: max|gpu - float64| = {far:.3e} (bound max(1e-3, 1e-3 |ref|))")
        bad = oracle.verify_results(np.ascontiguousarray(got_all), np.ascontiguousarray(exact, dtype=np.float32), 1e-3, 1e-3)
        assert bad == -1, (label, far, bad)


# ---- the library ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def compiled_module():
    """The compiled torch_ext extension beside libqmha.so, loaded once from its file."""
    import torch  # noqa: F401 -- the extension links against libtorch
    from quantizedmha_amd import _lib
    path = os.path.join(_lib.LIB_DIR, "torch_ext" + sysconfig.get_config_var("EXT_SUFFIX"))
    spec = importlib.util.spec_from_file_location("torch_ext", path)
    compiled = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(compiled)
    return compiled


@contextlib.contextmanager
def overlap_chunks(chunks):
    """qmha_set_overlap_chunks(chunks) around the body, which gets the library; the previous value comes back after."""
    from quantizedmha_amd import _lib
    lib = _lib.load()
    prev = lib.qmha_set_overlap_chunks(chunks)
    try:
        yield lib
    finally:
        lib.qmha_set_overlap_chunks(prev)


def c_solve(entry, variant, t, h, flags, h_kv=None, ws=None, ws_bytes=None, stream=None, expect=0):
    """qmha_solve_<entry> (`opts`: square; `rect`; `gqa`: with h_kv) on device tensors t = [Q [B, Nq, h d], K, V
    [B, Nk, ..]], with library-owned scratch or the caller's `ws` (stated as ws_bytes, default all of it); the status
    must be `expect`.  Returns O (numpy) through the guard, after a sync."""
    import torch
    from quantizedmha_amd import _lib
    lib = _lib.load()
    Q, K, V = t
    g = Guarded(Q)
    rows = (Q.shape[1],) if entry == "opts" else (Q.shape[1], K.shape[1])
    heads = (h, h_kv) if entry == "gqa" else (h,)
    st = getattr(lib, "qmha_solve_" + entry)(
        Q.data_ptr(), K.data_ptr(), V.data_ptr(), g.out.data_ptr(), Q.shape[0], *rows, Q.shape[-1], *heads,
        _lib.VARIANTS[variant], flags, ws.data_ptr() if ws is not None else None,
        (ws.numel() if ws_bytes is None else ws_bytes) if ws is not None else 0, stream)
    torch.cuda.synchronize()
    assert st == expect, (entry, st, expect, lib.qmha_last_error().decode())
    return g.result()


# ---- the K/V cache ---------------------------------------------------------------------------------------------------
def new_cache(dev, variant, B, cap, d, h, h_kv=None, mod=None):
    """KVCache, or GroupedKVCache with h_kv, of the ctypes binding or of `mod` (the compiled module)."""
    if mod is None:
        from quantizedmha_amd import torch_ext as mod
    if h_kv is None:
        return mod.KVCache(B, cap, h * d, h, variant, str(dev))
    return mod.GroupedKVCache(B, cap, h * d, h, h_kv, variant, str(dev))


def attend(cache, Q, causal=True, lens=None):
    """cache.attend, or attend_varlen with device lengths `lens`, through the guard; O (numpy) after a sync."""
    g = Guarded(Q)
    if lens is None:
        cache.attend(Q, causal=causal, out=g.buf[:g.n])
    else:
        cache.attend_varlen(Q, lens, causal=causal, out=g.buf[:g.n])
    return g.result()


def cache_layout(cache):
    """The byte layout of cache.mem, the workspace carve at N = cap: {array: (offset, bytes per slice)}.  An array holds
    B h_kv slices -- one per (sequence, K/V head), sequence-major -- back to back and starts on a multiple of 256."""
    al = lambda x: -(-x // 256) * 256  # noqa: E731
    slices, cap, d = cache.B * cache.num_kv_heads, cache.cap, cache.d_model // cache.num_heads
    if cache.kernel == INT8:
        e, s = al(slices * cap * d), al(slices * (cap // 32) * 4)
        layout = {"Ki": (0, cap * d), "Vh": (e, 2 * cap * d), "sK": (3 * e, (cap // 32) * 4), "sV": (3 * e + s, (cap // 32) * 4)}
        total = 3 * e + 2 * s
    else:
        e = al(2 * slices * cap * d)
        layout = {"Kh": (0, 2 * cap * d), "Vt": (e, 2 * cap * d)}
        total = 2 * e
    assert cache.mem.numel() == total, (cache.kernel, cache.mem.numel(), total)
    return layout


def cache_array(cache, name, dtype):
    """Array `name` of cache_layout as a view of cache.mem: [B h_kv, elements of dtype per slice]."""
    off, per = cache_layout(cache)[name]
    slices = cache.B * cache.num_kv_heads
    return cache.mem[off:off + slices * per].view(dtype).view(slices, -1)


def seq_slices(cache, b):
    """Byte ranges of sequence b in cache.mem: its h_kv slices of every array, in cache_layout's order."""
    hk = cache.num_kv_heads
    return [slice(off + b * hk * per, off + (b + 1) * hk * per) for off, per in cache_layout(cache).values()]
