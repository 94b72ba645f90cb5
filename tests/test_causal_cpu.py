"""CPU tests of the causal feature: the numpy restatement the GPU tests use as their int8
reference (tests/causal_ref.py) is held to the C oracle and to float64 masked attention, the C-ABI's flag
checks fail before any launch, and the bindings accept `causal=`.  No kernel is launched here."""
import ctypes
import inspect

import numpy as np
import pytest

from tests import causal_ref as cr

ALL_INT8_CASES = cr.CASES + cr.CASES_INT8_D32


@pytest.fixture(scope="module")
def built():
    from tools.build import build
    build(verbose=False)
    return True


@pytest.mark.parametrize("N,d_model,h,B,dist,seed", ALL_INT8_CASES)
def test_restatement_equals_oracle_without_mask(oracle_mod, N, d_model, h, B, dist, seed):
    """causal=False is the C oracle (oracle/qmha_oracle.c fa_int8_item) up to numpy's exp against libm's
    expf: every element within two one-flip units + 5e-5, the bound the GPU is held to."""
    Q, K, V = cr.inputs(N, d_model, B, dist, seed)
    got, unit = cr.fa_int8(oracle_mod, Q, K, V, d_model, h, causal=False)
    ref = oracle_mod.fa_int8(Q, K, V, d_model, h)
    err = np.abs(got.astype(np.float64) - ref)
    tol = 2.0 * cr.per_element(unit, d_model // h) + 5e-5
    print(f"N={N} d={d_model // h}: max|restatement - oracle| = {err.max():.2e}, worst err/tol = {(err / tol).max():.3f}")
    assert (err <= tol).all(), (float(err.max()), float((err / tol).max()))


@pytest.mark.parametrize("N,d_model,h,B,dist,seed", ALL_INT8_CASES)
def test_causal_restatement_within_quantisation_budget(oracle_mod, N, d_model, h, B, dist, seed):
    """causal=True against float64 masked attention.  Rows >= 32: the project's 5e-3 int8 budget.  Rows < 32
    average so few keys (row 0: one) that V's own quantisation step shows: within 1.5 steps of V's first
    group, 1.5 * absmax(V_head[0:32]) / 127 -- a property of the contract, not of a kernel."""
    d = d_model // h
    Q, K, V = cr.inputs(N, d_model, B, dist, seed)
    got, _ = cr.fa_int8(oracle_mod, Q, K, V, d_model, h, causal=True)
    err = np.abs(got - cr.attention_f64(Q, K, V, d_model, h, causal=True))
    step = np.abs(V.reshape(B, N, h, d)[:, :32]).max(axis=(1, 3)) / 127.0  # [B, h]
    early = (err[:, :32].reshape(B, 32, h, d) / step[:, None, :, None]).max()
    late = err[:, 32:].max() if N > 32 else 0.0
    print(f"N={N} d={d}: rows >= 32 max err {late:.2e}; rows < 32 worst {early:.2f} V steps")
    assert late <= 5e-3, late
    assert early <= 1.5, early


def test_mask_semantics_of_the_restatement(oracle_mod):
    """Row 0 sees key 0 alone: the dequantised V[0] when its p is the tile's largest (Pi = 127 and
    sP = 1/127 cancel), which a zero query row makes certain (score 0 = m0, p = 1; with a negative score
    p < 1 while another row of the tile has p = 1, and Pi = rint(127 p) carries up to 0.4 % rounding).
    Negating K and V from row j0 on -- no absmax, so no scale and no earlier byte, changes -- leaves every
    row < j0 bit-identical."""
    N, d_model, h = 96, 64, 2
    d = d_model // h
    Q, K, V = cr.inputs(N, d_model, 1, "normal", 7)
    Q[:, 0] = 0.0
    base, _ = cr.fa_int8(oracle_mod, Q, K, V, d_model, h, causal=True)
    Vi, sV = oracle_mod.quantize_heads(V, d_model, h)
    for k in range(h):
        np.testing.assert_allclose(base[0, 0, k * d:(k + 1) * d], Vi[0, k, 0].astype(np.float32) * sV[0, k, 0], rtol=1e-6)
    j0 = 45
    K2, V2 = K.copy(), V.copy()
    K2[:, j0:] *= -1
    V2[:, j0:] *= -1
    neg, _ = cr.fa_int8(oracle_mod, Q, K2, V2, d_model, h, causal=True)
    assert np.array_equal(neg[:, :j0], base[:, :j0])
    assert (neg[:, j0:] != base[:, j0:]).any(axis=-1).all()


# ---- C-ABI argument checks: they fail before any launch, so no device is needed ------------------------
CAUSAL = 1
NOSYS_CASES = [  # (variant id, name, d_model, h)
    (0, "fa", 128, 2),
    (3, "unfused", 128, 2),
    (4, "fa_mfma", 128, 2),
    (5, "fa_tc_int8_pt", 128, 2),
    (2, "fa_tc_int8_b", 192, 2),  # d = 96
    (1, "fa_tc_v1a", 192, 2),     # d = 96
    (1, "fa_tc_v1a", 64, 2),      # d = 32: int8 only
    (2, "fa_tc_int8_b", 512, 2),  # d = 256
]


def test_unknown_flag_bits_are_invalid(built):
    from quantizedmha_amd import _lib
    lib = _lib.load()
    dummy = ctypes.c_void_p(0x1000)  # never dereferenced: checks run first
    for flags in (2, 3, 0x80000000):
        st = lib.qmha_solve_opts(dummy, dummy, dummy, dummy, 1, 128, 128, 2, 2, flags, None, 0, None)
        assert st == 1, (flags, st)
        assert "flag" in lib.qmha_last_error().decode()
    # the shape checks of qmha_solve_ex come first and still apply
    st = lib.qmha_solve_opts(dummy, dummy, dummy, dummy, 1, 100, 128, 2, 2, CAUSAL, None, 0, None)
    assert st == 1 and "multiple of 32" in lib.qmha_last_error().decode()


@pytest.mark.parametrize("vid,name,d_model,h", NOSYS_CASES)
def test_causal_unsupported_combinations_are_nosys(built, vid, name, d_model, h):
    from quantizedmha_amd import _lib
    lib = _lib.load()
    dummy = ctypes.c_void_p(0x1000)
    for ws in (None, dummy):  # library-owned and caller-owned workspace forms
        st = lib.qmha_solve_opts(dummy, dummy, dummy, dummy, 1, 128, d_model, h, vid, CAUSAL, ws, 1 << 30, None)
        assert st == 4, st
        msg = lib.qmha_last_error().decode()
        assert name in msg and f"d = {d_model // h}" in msg, msg


def test_python_bindings_accept_causal():
    """`causal` is the trailing keyword, default False, of every binding; reference call sites are unchanged."""
    from quantizedmha_amd import jax_binding, jax_ext, shard, torch_ext
    for fn in (torch_ext.flash_solve, jax_ext.flash_solve, jax_binding.flash_solve_jax, shard.solve_sharded,
               shard.solve_shard_gather):
        params = list(inspect.signature(fn).parameters.values())
        assert params[-1].name == "causal" and params[-1].default is False, fn
    assert [p.name for p in inspect.signature(torch_ext.flash_solve).parameters.values()][:6] == \
        ["Q", "K", "V", "d_model", "num_heads", "kernel"]


def test_torch_bindings_take_causal_and_still_work_without_it(built):
    """Both torch bindings reach their own argument checks with and without `causal` (a binding that did
    not know the keyword would raise TypeError instead)."""
    torch = pytest.importorskip("torch")
    import importlib.util
    import os
    import sysconfig
    from quantizedmha_amd import _lib, torch_ext
    q = torch.zeros(32, 32)
    for kw in ({}, {"causal": True}, {"causal": False}):
        with pytest.raises(RuntimeError, match="Inputs must be CUDA tensors"):
            torch_ext.flash_solve(q, q, q, 32, 1, **kw)
    path = os.path.join(_lib.LIB_DIR, "torch_ext" + sysconfig.get_config_var("EXT_SUFFIX"))
    spec = importlib.util.spec_from_file_location("torch_ext", path)
    compiled = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(compiled)
    assert "causal" in compiled.flash_solve.__doc__
    for kw in ({}, {"causal": True}, {"kernel": "fa_tc_v1a", "causal": True}):
        with pytest.raises(RuntimeError, match="Inputs must be CUDA tensors"):
            compiled.flash_solve(q, q, q, 32, 1, **kw)


def test_shard_passes_causal_to_the_solve():
    """The batch-shard path hands `causal=True` to the solve (here a CPU stand-in that honours it) and leaves
    a stand-in without the keyword alone when the flag is off.  Single process: the mask is per sequence, so
    sharding the batch does not interact with it (the gloo tests of tests/test_dist.py cover the exchange)."""
    torch = pytest.importorskip("torch")
    from quantizedmha_amd import shard
    Q, K, V = (torch.from_numpy(x) for x in cr.inputs(64, 64, 2, "normal", 5))

    def stand_in(q, k, v, d_model, h, kernel, causal=False):
        return torch.from_numpy(cr.attention_f64(q.numpy(), k.numpy(), v.numpy(), d_model, h, causal)).float()

    def old_stand_in(q, k, v, d_model, h, kernel):
        return stand_in(q, k, v, d_model, h, kernel)

    full = shard.solve_sharded(Q, K, V, 64, 2, solve_fn=stand_in)
    masked = shard.solve_sharded(Q, K, V, 64, 2, solve_fn=stand_in, causal=True)
    assert torch.equal(full, shard.solve_sharded(Q, K, V, 64, 2, solve_fn=old_stand_in))
    assert torch.equal(masked, stand_in(Q, K, V, 64, 2, "fa_tc_int8_b", causal=True))
    assert not torch.equal(masked, full)
    out = torch.empty_like(Q)
    shard.solve_shard_gather(Q, K, V, 64, 2, batch=2, solve_fn=stand_in, out=out, causal=True)
    assert torch.equal(out, masked)
