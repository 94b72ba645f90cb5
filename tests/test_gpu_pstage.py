"""The P stage of the per-block int8 kernels on the GPU, checked per tile.

qmha_debug_fa_int8_pstage runs the dumping twin of the kernel a call would launch -- the pipelined kernel
(d = 32 / 64 / 128), the one-tile kernel (other head sizes, N = 32), the causal / rectangular kernel -- and every
case of tests/pstage_ref.py's CASES holds its dump to the restatement there: S, Qi, sQ, m, T and the untouched tiles
exactly (A, B, E, H), sP, Pi, l and O within the bounds derived there (C, D, F, G).  The twin's O must also be the
shipped kernel's O, bit for bit.  The observed maxima and the excused Pi counts are printed in pytest's terminal
summary (tests/parity_log.py).
"""
import numpy as np
import pytest

from oracle import oracle
from tests import parity_log
from tests import pstage_ref as ps
from tests.gpu_support import INT8, dev, to_dev  # noqa: F401

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.mark.parametrize("case", ps.CASES, ids=lambda c: c.label)
def test_pstage(dev, case):
    from quantizedmha_amd import torch_ext
    Q, K, V = case.build()
    d_model, h = case.d_model, case.h
    assert ps.kind_of(Q.shape[1], K.shape[1], d_model // h, case.causal) == case.kind, "the case no longer reaches its kernel"
    t = to_dev(dev, Q, K, V)
    O, dump = torch_ext.debug_fa_int8_pstage(t[0], t[1], t[2], d_model, h, causal=case.causal)
    shipped = torch_ext.flash_solve_rect(t[0], t[1], t[2], d_model, h, INT8, causal=case.causal)
    torch.cuda.synchronize()
    dump = {k: v.cpu().numpy() for k, v in dump.items()}
    dump["O"] = O.cpu().numpy()
    assert np.array_equal(dump["O"].view(np.int32), shipped.cpu().numpy().view(np.int32)), "the twin's O is not the shipped kernel's"
    form = ps.form_of(case)
    rec = ps.restate(oracle, Q, K, V, d_model, h, form, case.causal)
    seen = ps.check_all(dump, rec, torch_ext.PSTAGE_SENTINEL)  # A, B, E, H: exact; C, D, F, G: raise outside their bounds
    excused, total = seen["D"]
    share, variant = excused / total, f"pstage {case.kind}"
    parity_log.record(f"{case.label} [C: sP, largest relative difference]", variant, seen["C"], share, ps.EPS_SP[form])
    parity_log.record(f"{case.label} [F: l, error / bound; D: {excused} of {total} Pi excused]", variant, seen["F"], share, 1.0)
    parity_log.record(f"{case.label} [G: O, error / bound]", variant, seen["G"], share, 1.0)
    if case.label in ps.REANCHORS:
        assert ps.reanchors(dump["m"], rec).max() >= 1, "the inputs no longer re-anchor"
    if case.label == "hard-pipe-underflow-d64":
        assert (dump["sP"] == ps.FLOOR["kfold"]).any(), "the inputs no longer reach the sP floor"
