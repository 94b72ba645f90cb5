"""CPU tests: pin the oracle (oracle/qmha_oracle.c) against the reference's own outputs.

* cpu_attention  == generate_golden.cpp cpu_mha goldens (bit-exact; produced by the
  reference generator compiled from /root/reference, tests/golden/make_golden.py)
* cpu_reference_rope == the reference's utils/verify.cu (bit-exact; committed c1 caches and,
  when oracle/_ref is built, the live reference library)
* fa_fp32 / fa_fp16 / fa_int8 restatements: all-ones KAT (drivers/main.cu:73-101), agreement
  with the goldens within each variant's error budget, exact integer pieces.
"""
import os

import numpy as np
import pytest

from tests.golden_io import CASES, GOLD, load_case, load_inputs_cache, load_ref_cache


@pytest.mark.parametrize("case", CASES)
def test_cpu_attention_matches_reference_golden_bitexact(oracle_mod, case):
    N, dm, h, Q, K, V, O = load_case(case)
    out = oracle_mod.cpu_attention(Q, K, V, dm, h)
    assert np.array_equal(out, O), np.abs(out - O).max()


def test_cpu_reference_rope_matches_reference_cache_bitexact(oracle_mod):
    N, dm, (Q, K, V) = load_inputs_cache(os.path.join(GOLD, "c1_verify", "input_random_N128_d128.bin"))
    _, _, ref = load_ref_cache(os.path.join(GOLD, "c1_verify", "ref_N128_d128.bin"))
    out = oracle_mod.cpu_reference_rope(Q, K, V, dm, 2)
    assert np.array_equal(out, ref)


def test_cpu_reference_rope_matches_live_reference(oracle_mod):
    """N(0, 1) inputs at N96 d_model64 h2: bit-exact against the reference's cpu_reference, whose output for
    these inputs is committed (tests/golden/rope_normal, written by make_golden.py from the reference library),
    and against the library itself wherever oracle/_ref is built."""
    rng = np.random.default_rng(7)
    N, dm, h = 96, 64, 2
    Q, K, V = (rng.standard_normal((N, dm)).astype(np.float32) for _ in range(3))
    sN, sdm, stored_in = load_inputs_cache(os.path.join(GOLD, "rope_normal", "input_normal_N96_d64.bin"))
    assert (sN, sdm) == (N, dm) and all(np.array_equal(a, b) for a, b in zip((Q, K, V), stored_in))
    _, _, stored = load_ref_cache(os.path.join(GOLD, "rope_normal", "ref_N96_d64.bin"))
    out = oracle_mod.cpu_reference_rope(Q, K, V, dm, h)
    assert np.array_equal(out, stored)
    if oracle_mod.ref_lib() is not None:
        assert np.array_equal(out, oracle_mod.ref_cpu_reference(Q, K, V, dm, h))


def test_input_generator_restatement_matches_committed_cache():
    """oracle/_ref/ref_inputs restates inputs/data.cu:9-30; its output is the committed cache."""
    N, dm, (Q, K, V) = load_inputs_cache(os.path.join(GOLD, "c1_verify", "input_random_N128_d128.bin"))
    assert (N, dm) == (128, 128)
    assert Q.min() >= 0 and Q.max() < 1 and K.std() > 0.25  # U[0,1)
    assert not np.array_equal(Q, K)


def test_all_ones_kat(oracle_mod):
    """The driver's correctness check: all-ones Q/K/V -> every output element is 1.0
    (drivers/main.cu:73-101 with tolerance max(1e-3, 1e-3*|ref|))."""
    _, _, ref = load_ref_cache(os.path.join(GOLD, "c1_ones", "ref_N128_d128.bin"))
    assert np.allclose(ref, 1.0, atol=1e-6)
    ones = np.ones((128, 128), np.float32)
    for fn in (oracle_mod.fa_int8, oracle_mod.fa_fp16, oracle_mod.fa_fp32, oracle_mod.cpu_attention):
        out = fn(ones, ones, ones, 128, 2)
        assert oracle_mod.verify_results(out, ref, 1e-3, 1e-3) == -1


@pytest.mark.parametrize("case,tol", [("medium", 5e-3), ("large", 5e-3), ("huge_1024", 5e-3)])
def test_fa_int8_within_quantisation_error_of_golden(oracle_mod, case, tol):
    N, dm, h, Q, K, V, O = load_case(case)
    out = oracle_mod.fa_int8(Q, K, V, dm, h)
    err = np.abs(out - O).max()
    assert err < tol, err
    assert err > 1e-5  # it really is quantised


@pytest.mark.parametrize("case", ["medium", "large", "huge_1024"])
def test_fa_fp16_within_reference_tolerance(oracle_mod, case):
    N, dm, h, Q, K, V, O = load_case(case)
    out = oracle_mod.fa_fp16(Q, K, V, dm, h)
    assert oracle_mod.verify_results(out, O, 1e-3, 1e-3) == -1  # verify.cu default tolerances


@pytest.mark.parametrize("case", ["medium", "large", "huge_1024"])
def test_fa_fp16_lazy_within_reference_tolerance(oracle_mod, case):
    """The fp16 kernel's own contract (lazy softmax base): inside the reference's verify tolerance
    against the goldens, and within the 2e-4 fp16 parity bound of the reference's algorithm (fa_fp16)."""
    N, dm, h, Q, K, V, O = load_case(case)
    out = oracle_mod.fa_fp16_lazy(Q, K, V, dm, h)
    assert oracle_mod.verify_results(out, O, 1e-3, 1e-3) == -1
    assert np.abs(out - oracle_mod.fa_fp16(Q, K, V, dm, h)).max() <= 2e-4


@pytest.mark.parametrize("case", ["medium", "large", "huge_1024"])
def test_fa_fp32_close_to_golden(oracle_mod, case):
    N, dm, h, Q, K, V, O = load_case(case)
    out = oracle_mod.fa_fp32(Q, K, V, dm, h)
    assert np.abs(out - O).max() < 1e-5


def test_quantiser_exact_semantics(oracle_mod):
    """fa_tc_int8_b.cu:104-140: sc = max(absmax/127, 1e-8), q = clamp(rint(v * (1/sc)))."""
    rng = np.random.default_rng(3)
    N, dm, h = 64, 64, 1
    X = (rng.standard_normal((N, dm)) * 0.7).astype(np.float32)
    X[5, 7] = 5.0  # group 0 absmax
    X[40:] = 0.0   # group 1 all zero -> 1e-8 floor
    Xi, sc = oracle_mod.quantize_heads(X, dm, h)
    g0 = X[:32]
    exp_sc0 = np.maximum(np.float32(np.abs(g0).max()) / np.float32(127.0), np.float32(1e-8))
    assert sc[0, 0, 0] == exp_sc0
    inv = np.float32(1.0) / exp_sc0
    q = np.clip(np.rint(g0 * inv), -128, 127).astype(np.int8)  # np.rint is half-to-even
    assert np.array_equal(Xi[0, 0, :32], q)
    assert Xi.reshape(N, dm)[5, 7] == 127
    # group 1 rows 32..39 random, 40..63 zero
    g1 = X[32:]
    sc1 = np.maximum(np.float32(np.abs(g1).max()) / np.float32(127.0), np.float32(1e-8))
    assert sc[0, 0, 1] == sc1


def test_qk_int32_exact(oracle_mod):
    rng = np.random.default_rng(11)
    Qi = rng.integers(-128, 128, (64, 64), dtype=np.int8)
    Ki = rng.integers(-128, 128, (64, 64), dtype=np.int8)
    S = oracle_mod.qk_int32(Qi, Ki)
    assert np.array_equal(S, Qi.astype(np.int32) @ Ki.astype(np.int32).T)


def test_f16_conversion_is_round_to_nearest_even(oracle_mod):
    rng = np.random.default_rng(5)
    vals = np.concatenate([rng.standard_normal(2000).astype(np.float32) * 10,
                           np.array([0.0, -0.0, 1.0, 65504.0, 65520.0, 1e-8, 6e-5, 2 ** -24, 3 * 2 ** -25,
                                     1.0 + 2 ** -11, 1.0 + 3 * 2 ** -11], np.float32)])
    for v in vals:
        assert oracle_mod.f32_to_f16_bits(v) == int(np.float32(v).astype(np.float16).view(np.uint16)), v


def test_verify_results_semantics_match_reference(oracle_mod):
    a = np.ones(16, np.float32)
    b = a.copy()
    assert oracle_mod.verify_results(a, b) == -1
    b[3] = 1.0 + 2e-3
    assert oracle_mod.verify_results(a, b) == 3
    b[3] = np.nan
    assert oracle_mod.verify_results(a, b) == 3
    L = oracle_mod.ref_lib()
    if L is not None:
        import ctypes
        p = lambda x: x.ctypes.data_as(ctypes.POINTER(ctypes.c_float))  # noqa: E731
        c = a.copy()
        c[2] = 1.0005
        assert L.ref_verify_results(p(c), p(a), 16, 1e-3, 1e-3) == 1
        c[2] = 1.002
        assert L.ref_verify_results(p(c), p(a), 16, 1e-3, 1e-3) == 0


def test_quant_small_fixture_is_not_int8_b_semantics(oracle_mod):
    """generate_golden.cpp:163-187 writes int8 Q with a fixed 0.05 scale and std::round;
    documents why it cannot pin the per-block int8_b quantiser."""
    d = os.path.join(GOLD, "quant_small")
    Q = np.fromfile(os.path.join(d, "Q.f32.bin"), np.float32)
    Qi = np.fromfile(os.path.join(d, "Q.int8.bin"), np.int8)
    ref = np.clip(np.where(Q / 0.05 >= 0, np.floor(Q / np.float32(0.05) + 0.5), np.ceil(Q / np.float32(0.05) - 0.5)),
                  -128, 127).astype(np.int8)
    assert np.array_equal(Qi, ref)


# ---- fa_tc_int8_pt (per-tensor mode; no reference counterpart: pinned by the KAT, the error
# budget against the goldens, exact quantiser checks and an independent numpy restatement)

def test_int8_pt_all_ones_kat(oracle_mod):
    ones = np.ones((128, 128), np.float32)
    out = oracle_mod.fa_int8_pt(ones, ones, ones, 128, 2)
    _, _, ref = load_ref_cache(os.path.join(GOLD, "c1_ones", "ref_N128_d128.bin"))
    assert oracle_mod.verify_results(out, ref, 1e-3, 1e-3) == -1


@pytest.mark.parametrize("case", ["medium", "large", "huge_1024"])
def test_fa_int8_pt_within_quantisation_error_of_golden(oracle_mod, case):
    N, dm, h, Q, K, V, O = load_case(case)
    out = oracle_mod.fa_int8_pt(Q, K, V, dm, h)
    err = np.abs(out - O).max()
    assert 1e-5 < err < 5e-3, err


def test_int8_pt_quantiser_semantics(oracle_mod):
    """One scale per (sequence, head) slice: sc = max(absmax(slice)/127, 1e-8), x_i8 =
    clamp(rint(x * (1/sc))); where every 32-row group holds the slice's absmax the bytes equal the
    per-block quantiser's."""
    rng = np.random.default_rng(5)
    B, N, dm, h = 2, 96, 64, 2
    d = dm // h
    X = (rng.standard_normal((B, N, dm)) * 0.5).astype(np.float32)
    X[1, :, d:] = 0.0  # an all-zero slice -> the 1e-8 floor
    Xi, sc = oracle_mod.quantize_heads_pt(X, dm, h)
    assert sc.shape == (B, h) and Xi.shape == (B, h, N, d)
    for b in range(B):
        for k in range(h):
            sl = X[b, :, k * d:(k + 1) * d]
            s = np.maximum(np.float32(np.abs(sl).max()) / np.float32(127.0), np.float32(1e-8))
            assert sc[b, k] == s
            q = np.clip(np.rint(sl * (np.float32(1.0) / s)), -128, 127).astype(np.int8)
            assert np.array_equal(Xi[b, k], q)
    Y = X.copy()
    Y[:, ::32, 0] = 9.0  # the same absmax in every group of head 0
    Yi_pt, _ = oracle_mod.quantize_heads_pt(Y, dm, h)
    Yi_pb, _ = oracle_mod.quantize_heads(Y, dm, h)
    assert np.array_equal(Yi_pt[:, 0], Yi_pb[:, 0])


def _pt_score_constant(sQ, sK, d):
    """The kernel's base-2 score constant: RN22(sQ * RN(RN(1/sqrt(d)) * log2 e) * sK) in float32."""
    f = np.float32
    c_log2 = (f(1.0) / np.sqrt(f(d))) * f(1.4426950408889634)
    c = np.array([(f(sQ) * c_log2) * f(sK)], np.float32).view(np.uint32)
    return ((c + np.uint32(2)) & np.uint32(0xFFFFFFFC)).view(np.float32)[0]


def _tree_sum16_rows(p):
    """The kernels' tree_sum16 order over the 16 columns of p (float32)."""
    a = (p[:, 0] + p[:, 1]) + (p[:, 2] + p[:, 3])
    b = (p[:, 4] + p[:, 5]) + (p[:, 6] + p[:, 7])
    c = (p[:, 8] + p[:, 9]) + (p[:, 10] + p[:, 11])
    d = (p[:, 12] + p[:, 13]) + (p[:, 14] + p[:, 15])
    return (a + b) + (c + d)


def _tree_sum8_rows(p):
    """The 16x16 kernels' eight-key tree: ((p0 + p1) + (p2 + p3)) + ((p4 + p5) + (p6 + p7))."""
    return ((p[:, 0] + p[:, 1]) + (p[:, 2] + p[:, 3])) + ((p[:, 4] + p[:, 5]) + (p[:, 6] + p[:, 7]))


def _np_fa_int8_pt(Q, K, V, h):
    """numpy restatement of oracle_fa_int8_pt for one sequence (base 2, the kernel's score constant;
    float32 arithmetic except x = S * c - m, rounded once from float64 like the kernel's fma)."""
    f = np.float32
    N, dm = Q.shape
    d = dm // h
    out = np.zeros_like(Q)
    for k in range(h):
        sl = slice(k * d, (k + 1) * d)
        qs = []
        for X in (Q, K, V):
            s = np.maximum(f(np.abs(X[:, sl]).max()) / f(127.0), f(1e-8))
            qs.append((np.clip(np.rint(X[:, sl] * (f(1.0) / s)), -128, 127).astype(np.int64), s))
        (Qi, sQ), (Ki, sK), (Vi, sV) = qs
        c = _pt_score_constant(sQ, sK, d)
        if d == 64:  # the 16x16 kernel's lane quarters (keys kap16(j >> 2, 4 g + (j & 3)), pairwise tree)
            halves = [np.array([16 * ((4 * g + (j & 3)) >> 3) + 4 * (((4 * g + (j & 3)) >> 2) & 1) + (j & 3) + 8 * (j >> 2)
                                for j in range(8)]) for g in range(4)]
        else:  # the 32x32 kernel's lane halves
            halves = [np.array([(i & 3) + 8 * (i >> 2) + 4 * hh for i in range(16)]) for hh in range(2)]
        cap = f(2047.0) / f(127.0)
        for g in range(N // 32):
            rows = slice(32 * g, 32 * g + 32)
            O = np.zeros((32, d), f)
            l = np.zeros((32, len(halves)), f)
            m = np.zeros(32, f)
            for t in range(N // 32):
                cols = slice(32 * t, 32 * t + 32)
                S = Qi[rows] @ Ki[cols].T
                xm = S.max(axis=1).astype(f) * c
                if t == 0:  # lazy base (r06): tile 0 takes max(m0, row max) ...
                    m = np.maximum(m, xm).astype(f)

                def tile_p(base):
                    x = (S.astype(np.float64) * np.float64(c) - base[:, None].astype(np.float64)).astype(f)
                    p = np.exp2(x).astype(f)
                    return p, np.stack([_tree_sum16_rows(p[:, hv]) if len(hv) == 16 else _tree_sum8_rows(p[:, hv])
                                        for hv in halves], axis=1)
                p, ts = tile_p(m)
                alpha = np.ones(32, f)
                if t > 0:  # ... later tiles move it to the row max when a key half sums above the cap
                    rb = (ts > cap).any(axis=1)
                    alpha = np.where(rb, np.exp2(m - xm), f(1.0)).astype(f)
                    m = np.where(rb, xm, m).astype(f)
                    p2, ts2 = tile_p(m)
                    p, ts = np.where(rb[:, None], p2, p), np.where(rb[:, None], ts2, ts)
                l = (alpha[:, None] * l + ts).astype(f)
                Pi = np.minimum(np.rint(p * f(127.0)), 2047).astype(np.int64)
                O = O * alpha[:, None] + (Pi @ Vi[cols]).astype(f)
            l = (l[:, 0] + l[:, 1]) + (l[:, 2] + l[:, 3]) if len(halves) == 4 else l[:, 0] + l[:, 1]
            out[rows, sl] = np.where(l[:, None] > 1e-20, O * (sV / f(127.0)) / l[:, None], 0)
    return out


@pytest.mark.parametrize("dm", [64, 128])  # d = 32 (lane halves) and d = 64 (the 16x16 kernel's quarters)
def test_fa_int8_pt_matches_numpy_restatement(oracle_mod, dm):
    rng = np.random.default_rng(13)
    N, h = 128, 2
    Q, K, V = (rng.standard_normal((N, dm)).astype(np.float32) for _ in range(3))
    got = oracle_mod.fa_int8_pt(Q, K, V, dm, h)
    ref = _np_fa_int8_pt(Q, K, V, h)
    err = np.abs(got - ref)
    # expf vs numpy's exp and the row-sum order differ by ulps, which could flip a Pi at a .5
    # boundary; this seed has none (observed 1.2e-7)
    assert err.max() < 1e-6, err.max()
