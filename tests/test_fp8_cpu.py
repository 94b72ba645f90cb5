"""CPU tests of the e4m3 K/V cache variant fa_tc_fp8: the interface, the layout, the host refusals (every
host check runs before any HIP call, so dummy pointers reach them), the kernel instances, the LDS swizzle and the
contract's restatement (tests/fp8_ref.py) against float64."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tests import fp8_ref

FP8, V1A, CAUSAL = 6, 1, 1
MEM, DUMMY = ctypes.c_void_p(0x10000), ctypes.c_void_p(0x1000)  # aligned, never dereferenced: checks run first


@pytest.fixture(scope="module")
def lib():
    from tools.build import build
    build(verbose=False)
    from quantizedmha_amd import _lib
    return _lib.load()


def make(lib, variant=FP8, paged=False):
    h = ctypes.c_void_p()
    if paged:
        st = lib.qmha_kv_cache_create_paged(ctypes.byref(h), MEM, 1 << 30, 2, 8, 64, 4, 128, 2, 2, variant)
    else:
        st = lib.qmha_kv_cache_create(ctypes.byref(h), MEM, 1 << 30, 2, 256, 128, 2, variant)
    assert st == 0, lib.qmha_last_error()
    return h


def test_interface_and_cache_bytes(lib):
    from quantizedmha_amd import _lib
    assert _lib.VARIANTS["fa_tc_fp8"] == FP8 == lib.qmha_variant_from_name(b"fa_tc_fp8") and lib.qmha_variant_name(FP8) == b"fa_tc_fp8"
    assert _lib.SIGNATURES["qmha_kv_cache_set_scales"] == (ctypes.c_int, [ctypes.c_void_p] + [ctypes.c_float] * 3)
    assert lib.qmha_workspace_size(16, 4096, 1024, 16, FP8) == 0
    assert lib.qmha_kv_cache_bytes(16, 4096, 1024, 16, FP8) * 2 == lib.qmha_kv_cache_bytes(16, 4096, 1024, 16, V1A) == 268435456
    assert lib.qmha_kv_cache_bytes(1, 32, 192, 3, FP8) == 2 * 6144  # 3 slices of 32 * 64 bytes
    assert lib.qmha_kv_cache_bytes(3, 32, 64, 1, FP8) == 2 * 6144
    assert lib.qmha_kv_cache_bytes(1, 32, 64, 1, FP8) == 2 * 2048 and lib.qmha_kv_cache_bytes(1, 96, 128, 1, FP8) == 2 * 12288
    assert lib.qmha_kv_cache_paged_bytes(5, 64, 256, 4, 2, FP8) == 2 * 5 * 2 * 64 * 64
    assert lib.qmha_kv_cache_bytes(1, 32, 32, 1, FP8) == 0  # d = 32 is not built
    c = make(lib)
    assert lib.qmha_kv_cache_tail_bytes(c) == 0 and lib.qmha_kv_cache_attach_tail(c, None, 0) == 0
    lib.qmha_kv_cache_destroy(c)


def test_host_refusals(lib):
    def refused(st, status, *words):
        msg = lib.qmha_last_error().decode()
        assert st == status and all(w in msg for w in words), (st, msg)

    refused(lib.qmha_solve_ex(DUMMY, DUMMY, DUMMY, DUMMY, 1, 128, 128, 2, FP8, None), 4, "fa_tc_fp8 is a K/V cache variant")
    refused(lib.qmha_solve_rect(DUMMY, DUMMY, DUMMY, DUMMY, 1, 64, 128, 128, 2, FP8, CAUSAL, None, 0, None), 4, "K/V cache variant")
    h = ctypes.c_void_p()
    refused(lib.qmha_kv_cache_create(ctypes.byref(h), MEM, 1 << 30, 2, 256, 64, 2, FP8), 4, "fa_tc_fp8 at d = 32", "d = 64, 128")
    refused(lib.qmha_kv_cache_create(ctypes.byref(h), MEM, 100, 2, 256, 128, 2, FP8), 1, "too small", str(2 * 2 * 2 * 256 * 64))
    c, p = make(lib), make(lib, paged=True)
    a = (DUMMY, DUMMY, 1, DUMMY)  # Q, O, Nq, lens
    refused(lib.qmha_attend_cached_tokens_window(c, *a, 32, CAUSAL, None), 4, "attend_tokens_window", "sliding window", "fa_tc_fp8")
    refused(lib.qmha_attend_cached_tokens_split(c, *a, 64, DUMMY, 1 << 30, CAUSAL, None), 4, "attend_tokens_split", "split-KV")
    refused(lib.qmha_kv_cache_append_packed(c, DUMMY, DUMMY, 4, 2, DUMMY, DUMMY, None), 4, "append_packed", "packed batch")
    refused(lib.qmha_attend_cached_paged_packed(p, DUMMY, DUMMY, 4, 2, DUMMY, DUMMY, DUMMY, CAUSAL, None), 4, "packed batch")
    assert lib.qmha_kv_cache_set_scales(c, 0.5, 2.0, 0.25) == 0
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        refused(lib.qmha_kv_cache_set_scales(c, 1.0, bad, 1.0), 1, "finite and > 0")
    f16 = make(lib, V1A)
    refused(lib.qmha_kv_cache_set_scales(f16, 1.0, 1.0, 1.0), 1, "fa_tc_v1a cache", "fa_tc_fp8")
    for x in (c, p, f16):
        lib.qmha_kv_cache_destroy(x)


def test_one_instance_per_geometry_or_policy_and_d(lib):
    syms = subprocess.run(["nm", "-C", os.path.join(os.path.dirname(fp8_ref.__file__), "..", "quantizedmha_amd", "lib", "libqmha.so")], capture_output=True, text=True, check=True).stdout
    got = sorted(set(re.findall(r"__device_stub__(qmha_(?:fa_fp8|fp8_kv)_kernel<.*?>)\(", syms)))
    want = [f"qmha_fa_fp8_kernel<qmha::{g}, {d}>" for g in ("Grouped", "Varlen", "Ragged", "Paged") for d in (64, 128)]
    want += [f"qmha_fp8_kv_kernel<qmha::{p}, {d}>" for d in (64, 128) for p in
             ("LenRow, qmha::SliceRows", "PosRow<true>, qmha::SliceRows", "PosRow<false>, qmha::SliceRows", "PosRow<false>, qmha::PoolRows")]
    assert got == sorted(want), got


def test_lds_reads_are_conflict_free():
    """qmha_fa_fp8.hip's ds_read_b128 maps: K row 32 gi + kap16(kb, r16), chunk (4 kp + grp) ^ kswz16<D>; V^T line 16 mp + r16,
    chunk grp ^ vswz16(line).  Every 16-lane read group hits 16 distinct 16-byte slots; the block's map is a bijection."""
    groups = [list(range(0, 4)) + list(range(12, 16)) + list(range(20, 28)), list(range(4, 12)) + list(range(16, 20)) + list(range(28, 32))]
    groups += [[lane + 32 for lane in g] for g in groups]
    kap16 = lambda kb, m: 16 * (m >> 3) + 4 * ((m >> 2) & 1) + (m & 3) + 8 * kb  # noqa: E731
    kswz = {64: lambda r: 2 * ((r >> 4) & 1), 128: lambda r: ((r >> 1) & 1) ^ (2 * ((r >> 2) & 1)) ^ (4 * ((r >> 4) & 1))}
    vswz = lambda d: (2 * ((d >> 2) & 1)) ^ (3 * ((d >> 3) & 1))  # noqa: E731
    for D, f in kswz.items():
        for g in groups:
            for gi, kb, kp in np.ndindex(2, 2, D // 64):
                rows = [32 * gi + kap16(kb, lane & 15) for lane in g]
                assert len({(r * D // 16 + ((4 * kp + (lane >> 4)) ^ f(r))) % 16 for r, lane in zip(rows, g)}) == 16, (D, gi, kb, kp)
            for mp in range(D // 32):
                lines = [16 * mp + (lane & 15) for lane in g]
                assert len({(4 * ln + ((lane >> 4) ^ vswz(ln))) % 16 for ln, lane in zip(lines, g)}) == 16, (D, mp)
        assert sorted(fp8_ref.vt_offset(*np.meshgrid(np.arange(D), np.arange(32))).ravel()) == list(range(32 * D))


@pytest.mark.parametrize("dist", ["normal", "uniform"])
def test_restatement_against_float64(dist):
    """Each p is within 2^-4 of its value (3 mantissa bits, RNE) or, below e4m3's 2^-10 of the row's base 2^8, lost: so O
    is within 2^-4 max|v| + L 2^-18 max|v| of float64 attention on the same e4m3 operands."""
    from tests import rect_ref as rr
    (Nq, L, D), scales = (40, 100, 64), (0.3, 0.7, 1.9)
    Q, K, V = (x[0] for x in rr.inputs(Nq, L, D, 1, dist, 5))
    k8, _, v8 = fp8_ref.cache_arrays(K, V, L, scales[1], scales[2])
    q, k, v = (fp8_ref.decode(a).astype(np.float64) for a in (fp8_ref.encode(Q, scales[0]), k8, v8))
    O, l, vmax = fp8_ref.attend(q, k, v, L, scales)
    s = (q @ k[:L].T) * scales[0] * scales[1] / np.sqrt(D)
    s[np.arange(L)[None, :] > (np.arange(Nq) + L - Nq)[:, None]] = -np.inf
    p = np.exp(s - s.max(axis=1, keepdims=True))
    exact = scales[2] * (p @ v[:L]) / p.sum(axis=1, keepdims=True)
    assert (l >= 256).all() and np.abs(O - exact).max() <= (2.0 ** -4 + L * 2.0 ** -18) * vmax
