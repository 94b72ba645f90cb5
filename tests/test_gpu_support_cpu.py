"""What tests/gpu_support.py enforces, pinned on numpy arrays (the GPU test files all lean on that one copy): the int8
bound 2 u_r + 5e-5 and the fp16 bounds hold to the last ulp and fail just past it, on one element of many; a NaN or an
Inf fails; bit-identity notices a last-bit difference and a NaN in the reference; tests/parity_log.py gets the label,
the variant tag and the bound.  One GPU case: a write behind O's last row is noticed, an untouched guard passes.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import gpu_support as gs
from tests import parity_log
from tests.gpu_support import dev  # noqa: F401

SHAPE = (64, 32)
UNIT = np.full(SHAPE, 1e-3)
BOUND = 2.0 * 1e-3 + 5e-5  # float64, as assert_int8 computes it
ZERO = np.zeros(SHAPE)
TOL = 2.0 ** -10  # a power of two: float32 holds it, so |got - 0| == tol exactly


@pytest.fixture
def entries():
    """parity_log.ENTRIES, emptied for the test and put back afterwards."""
    saved = parity_log.ENTRIES[:]
    del parity_log.ENTRIES[:]
    yield parity_log.ENTRIES
    parity_log.ENTRIES[:] = saved


def one_off(base, value, dtype=np.float64):
    """[64, 32] of `base` with a single element set to `value`."""
    got = np.full(SHAPE, base, dtype=dtype)
    got[37, 11] = value
    return got


def test_int8_passes_one_ulp_inside_the_bound_everywhere(entries):
    got = np.full(SHAPE, np.nextafter(BOUND, 0.0))
    got[::2] *= -1.0
    gs.assert_int8("inside", got, ZERO, UNIT, "+t")
    label, tag, units, frac, bound = entries[0]
    assert (label, tag, bound) == ("inside [max error beyond 5e-5, in one-flip units]", gs.INT8 + "+t", 2.0)
    assert units == pytest.approx(2.0) and frac == 1.0 and len(entries) == 1


def test_int8_raises_on_one_element_just_outside(entries):
    with pytest.raises(AssertionError, match="outside"):
        gs.assert_int8("outside", one_off(0.0, BOUND + 1e-9), ZERO, UNIT, "+t")
    assert entries[0][2] > 2.0  # what was measured is recorded before the bound is applied
    gs.assert_int8("at the bound", one_off(0.0, BOUND), ZERO, UNIT, "+t")


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_int8_raises_on_one_non_finite_element(entries, bad):
    with pytest.raises(AssertionError, match="not finite"):
        gs.assert_int8("non-finite", one_off(0.0, bad), ZERO, UNIT, "+t")


def test_f16_passes_at_tol_and_raises_just_outside(entries):
    gs.assert_f16("at tol", np.full(SHAPE, TOL, dtype=np.float32), ZERO, TOL, "+t")
    assert entries == [("at tol (vs lazy contract)", gs.F16 + "+t", TOL, 1.0, TOL)]
    with pytest.raises(AssertionError, match="outside"):
        gs.assert_f16("outside", one_off(0.0, TOL + 1e-9, np.float32), ZERO, TOL, "+t")
    with pytest.raises(AssertionError, match="not finite"):
        gs.assert_f16("non-finite", one_off(0.0, np.nan, np.float32), ZERO, TOL, "+t")


def test_f16_exact_is_held_beside_the_contract(entries, oracle_mod):
    """One element 1.5e-3 from float64 where max(1e-3, 1e-3 |ref|) = 1e-3, with the contract met exactly."""
    got = one_off(0.0, 1.5e-3, np.float32)
    with pytest.raises(AssertionError, match="exact"):
        gs.assert_f16("exact", got, got.astype(np.float64), TOL, "+t", exact=ZERO)
    assert [(e[0], e[1], e[4]) for e in entries] == [("exact (vs lazy contract)", gs.F16 + "+t", TOL),
                                                     ("exact (vs float64)", gs.F16 + "+t", 1e-3)]
    gs.assert_f16("exact, inside", one_off(0.0, 0.9e-3, np.float32), ZERO, TOL, "+t", exact=ZERO)
    # got_all: the float64 bound is held on it and not on got
    with pytest.raises(AssertionError, match="got_all"):
        gs.assert_f16("got_all", np.zeros(SHAPE, np.float32)[:, :16], ZERO[:, :16], TOL, "+t", exact=ZERO, got_all=got)


def test_bits_raise_on_a_last_bit_and_on_a_nan_reference():
    want = np.full(SHAPE, 0.75, dtype=np.float32)
    gs.assert_bits("same", want.copy(), want)
    with pytest.raises(AssertionError, match="last bit"):
        gs.assert_bits("last bit", one_off(0.75, np.nextafter(np.float32(0.75), np.float32(1.0)), np.float32), want)
    nan = one_off(0.75, np.nan, np.float32)
    with pytest.raises(AssertionError, match="not finite"):
        gs.assert_bits("nan", nan.copy(), nan)
    with pytest.raises(AssertionError, match="not finite"):
        gs.assert_bits("inf", one_off(0.75, np.inf, np.float32), one_off(0.75, np.inf, np.float32))


def test_zeros_are_positive_zeros():
    gs.assert_zeros("zeros", np.zeros(SHAPE, np.float32))
    for bad in (-0.0, 1e-45, np.nan):
        with pytest.raises(AssertionError, match="zeros"):
            gs.assert_zeros("zeros", one_off(0.0, bad, np.float32))


def test_the_module_imports_without_torch():
    code = "import sys; sys.modules['torch'] = None; from tests import gpu_support as gs; print(gs.GUARD, gs.BUILT[0])"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=root)
    assert r.returncode == 0 and r.stdout.split()[0] == "7.25", r.stdout + r.stderr


@pytest.mark.gpu
def test_a_write_behind_the_last_row_is_noticed(dev):
    """An in-bounds assignment to one element of the guard's tail (the buffer is the test's own)."""
    import torch
    Q = torch.zeros((32, 64), dtype=torch.float32, device=dev)
    clean, hit = gs.Guarded(Q), gs.Guarded(Q)
    assert hit.buf.numel() == 64 * 64 and hit.out.shape == Q.shape
    hit.buf[hit.n + 31 * 64 + 5] = 0.0  # the last guard row
    with pytest.raises(AssertionError, match="O written past its last row"):
        hit.result()
    assert (clean.result() == gs.GUARD).all()

