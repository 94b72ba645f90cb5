"""CPU tests of the hard inputs of the fp8 cache kernels (tests/fp8_hard.py): the e4m3 reference against an integer
encoder of its own, the instrumented restatement against the plain ones, what every score family reaches at the shapes of
tests/test_gpu_fp8_hard.py, that the bound is usable on them, that every mutant of the restatement is caught by the comparison
the GPU file calls, and the stages its (lens, chunk_rows) set covers."""
import functools

import numpy as np
import pytest

from tests import decode_ref, fp8_ref
from tests import decode_window_ref as dwr
from tests import fp8_hard as H


def e4m3_rne(x):
    """e4m3fn bytes of float32 x, clamped to +-448, round to nearest even, in integers on the fp32 bit pattern."""
    bits = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.int64)
    sign, mag = (bits >> 31) << 7, np.minimum(bits & 0x7FFFFFFF, 0x43E00000)  # 0x43e00000: 448.0; inf and 1e30 clamp here
    e, sig = (mag >> 23) - 127, (mag & 0x7FFFFF) | 0x800000
    # normal (e >= -6): keep 3 mantissa bits, a carry runs into the exponent field; below: units of 2^-9, shift 14 - e
    shift = np.where(e >= -6, 20, np.minimum(14 - e, 40))
    q, rest, half = sig >> shift, sig & ((1 << shift) - 1), 1 << (shift - 1)
    q = q + ((rest > half) | ((rest == half) & (q & 1 == 1)))
    byte = np.where(e >= -6, ((e + 7) << 3) + (q - 8), q)
    return (np.where(mag >> 23 == 0, 0, byte) | sign).astype(np.uint8)  # an fp32 subnormal is far below 2^-10


def test_edge_table_holds_what_it_should():
    t, f = H.edge_table(), np.float32
    assert t.dtype == np.float32 and not np.isnan(t).any() and len(H.MAGS) == 127 and H.MAGS[-1] == 448 and H.MAGS[1] == 2.0 ** -9
    for v in list(H.MAGS) + [2.0 ** -10, np.nextafter(f(2.0 ** -10), f(1)), np.nextafter(f(2.0 ** -10), f(0)), 17.0, 19.0, 464.0, 480.0, 1e30,
                             np.inf, np.nextafter(f(448), f(np.inf)), 1e-45, np.nextafter(np.finfo(f).tiny, f(0))]:
        assert (t == f(v)).any() and (t == -f(v)).any(), v
    assert np.signbit(t[t == 0]).any() and not np.signbit(t[t == 0]).all()
    assert np.isfinite(H.edge_table(inf=False)).all() and len(H.edge_table(inf=False)) == len(t) - 2
    for d in (64, 128):  # every value in at least three (row mod 32, d) positions of a 224-row slice
        at, spots = H.place(np.arange(len(t)), H.CAP, d), {}
        for (r, c), i in np.ndenumerate(at):
            spots.setdefault(int(i), set()).add((r % 32, c))
        assert len(spots) == len(t) and min(len(s) for s in spots.values()) >= 3


@pytest.mark.parametrize("scale", [1.0, 0.3, 0.7, 1.9, 0.5])
def test_encode_against_an_integer_encoder(scale):
    t = H.edge_table()
    x = (t * np.float32(scale)).astype(np.float32)
    got, want = fp8_ref.encode(x, scale), e4m3_rne(x / np.float32(scale))
    assert np.array_equal(got, want), [(float(a), hex(b), hex(c)) for a, b, c in zip(x[got != want][:8], got[got != want], want[got != want])]
    if scale == 1.0:
        assert set(got) == set(range(0x7F)) | set(range(0x80, 0xFF))  # every finite byte, never the NaN byte
        assert np.array_equal(fp8_ref.decode(fp8_ref.encode(H.MAGS, 1.0)), H.MAGS) and np.array_equal(fp8_ref.encode(-H.MAGS, 1.0), np.arange(0x80, 0xFF))


def test_encode_spot_values():
    x = np.array([2.0 ** -10, 3 * 2.0 ** -10, 17.0, 19.0, 464.0, np.inf, -0.0, 16.0, 20.0, -np.inf, 1e-45, 5 * 2.0 ** -10], np.float32)
    want = [0x00, 0x02, 0x58, 0x5A, 0x7E, 0x7E, 0x80, 0x58, 0x5A, 0xFE, 0x00, 0x02]
    assert fp8_ref.encode(x, 1.0).tolist() == want and e4m3_rne(x).tolist() == want


@functools.lru_cache(maxsize=None)
def reach(name, d):
    """The counters of one family over every call tests/test_gpu_fp8_hard.py makes on it at head size d, per path."""
    n = {k: H.counters() for k in ("attend", "decode", "window")}
    for nq, lens in H.PREFILL:
        Q, K, V = H.family(name, d, 2, 2, nq, lens)
        for b, L in enumerate(lens):
            for k in range(2):
                H.attend(*(x[b][:, k * d:(k + 1) * d] for x in (Q, K, V)), L, H.SCALES, n=n["attend"])
    for h, hk, nq in H.HEADS:
        for lens in (H.lens_of(nq, "edge"), H.lens_of(nq, "mid")):
            Q, K, V = H.family(name, d, h, hk, nq, lens)
            for chunk in H.CHUNKS:
                H.decode(Q, K, V, lens, h, hk, H.SCALES, chunk, H.CAP, n=n["decode"])
                for window in H.WINDOWS:
                    H.decode(Q, K, V, lens, h, hk, H.SCALES, chunk, H.CAP, window, H.ramp(h), n=n["window"])
    return n


# family -> the counters it is there to reach, on every path named
REACHES = {
    "rise": {"rise_tiles": ("attend", "decode", "window")},
    "fall": {"still_tiles": ("attend", "decode", "window"), "p_subnormal": ("attend", "decode", "window"), "p_flushed": ("attend", "decode", "window")},
    "spike": {"alpha_underflow": ("attend", "decode", "window"), "merge_tiny": ("decode", "window")},
    "oddmax": {"merge_small": ("decode", "window"), "p_flushed": ("attend",)},
    "evenmax": {"merge_small": ("decode", "window"), "p_flushed": ("attend",)},
    "chunkmax": {"combine_tiny": ("decode", "window"), "alpha_underflow": ("attend",)},
    "superdiag": {"masked_above": ("attend", "decode", "window"), "empty_partials": ("window",)},
    "const": {"still_tiles": ("attend", "decode", "window"), "empty_partials": ("window",)},
    "clamp": {"saturated": ("attend", "decode", "window")},
    "zero_q": {"still_tiles": ("attend", "decode", "window")},
    "zero_v": {},  # its own assertion below
}


@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("name", H.FAMILIES)
def test_every_family_reaches_what_it_is_for(name, d):
    n = reach(name, d)
    print(name, d, {k: dict(v) for k, v in n.items()})
    for counter, paths in REACHES[name].items():
        for path in paths:
            assert n[path][counter] > 0, (name, d, path, counter)
    if name == "clamp":  # about half of the cached bytes
        assert 0.4 <= n["attend"]["saturated"] / n["attend"]["bytes"] <= 0.7
    if name in ("const", "zero_q"):  # the maximum never moves: the no-ballot path from the second tile to the end
        assert all(n[p]["rise_tiles"] == 0 for p in n)
    if name == "zero_v":  # V is 0 and the restatement's O exactly 0, on scores that move like any other family's
        (h, hk, nq), lens = H.HEADS[1], H.lens_of(5, "mid")
        Q, K, V = H.family(name, d, h, hk, nq, lens)
        assert not V.any() and K.std() > 0 and not H.decode(Q, K, V, lens, h, hk, H.SCALES, 64, H.CAP, 33, H.ramp(h))[0].any()
    if name == "rise":
        assert all(n[p]["rise_tiles"] > 10 * n[p]["still_tiles"] for p in ("attend", "decode"))  # all but a one-key tile or two


@pytest.mark.parametrize("name", ["spike", "superdiag", "fall"])
def test_instrumented_restatement_is_the_restatement(name):
    """Bit for bit in float64: fp8_ref.attend, decode_ref.decode and decode_window_ref.decode_window."""
    d, (h, hk, nq) = 64, H.HEADS[1]
    lens = H.lens_of(nq, "mid")
    Q, K, V = H.family(name, d, h, hk, nq, lens)
    for b, L in enumerate(lens):
        got = H.attend(Q[b][:, :d], K[b][:, :d], V[b][:, :d], L, H.SCALES, n=H.counters())
        want = fp8_ref.attend(*H.operands(Q[b][:, :d], K[b][:L, :d], V[b][:L, :d], L, H.SCALES), L, H.SCALES)
        assert all(np.array_equal(a, w) for a, w in zip(got, want))
    flat = lambda r: [r[0], *r[1], r[2], r[3]]  # noqa: E731
    for chunk in H.CHUNKS:
        got, want = H.decode(Q, K, V, lens, h, hk, H.SCALES, chunk, H.CAP, n=H.counters()), decode_ref.decode(Q, K, V, lens, h, hk, H.SCALES, chunk, H.CAP)
        assert all(np.array_equal(a, w, equal_nan=True) for a, w in zip(flat(got), flat(want)))
        for window, sinks in ((1, None), (33, H.ramp(h)), (100, H.ramp(h)), (1000, None)):
            got = H.decode(Q, K, V, lens, h, hk, H.SCALES, chunk, H.CAP, window, sinks, n=H.counters())
            want = dwr.decode_window(Q, K, V, lens, h, hk, H.SCALES, chunk, H.CAP, window, sinks)
            assert all(np.array_equal(a, w, equal_nan=True) for a, w in zip(flat(got), flat(want)))


@pytest.mark.parametrize("hnq", H.BIG_HEADS[1:])
def test_instrumented_restatement_is_the_restatement_at_the_multi_stage_shape(hnq):
    """The same at cap 768: chunk_rows 192 and 320, and the windowed forms of the GPU file."""
    d, (h, hk, nq), cap = 64, hnq, H.BIG_CAP
    lens = H.big_lens(nq)[2]
    Q, K, V = H.family("rise", d, h, hk, nq, lens, cap)
    flat = lambda r: [r[0], *r[1], r[2], r[3]]  # noqa: E731
    for chunk in (192, 320):
        got, want = H.decode(Q, K, V, lens, h, hk, H.SCALES, chunk, cap, n=H.counters()), decode_ref.decode(Q, K, V, lens, h, hk, H.SCALES, chunk, cap)
        assert all(np.array_equal(a, w, equal_nan=True) for a, w in zip(flat(got), flat(want)))
    for (window, chunk), sinks in zip(H.BIG_WINDOWS, (H.ramp(h), None, H.ramp(h), None)):
        got = H.decode(Q, K, V, lens, h, hk, H.SCALES, chunk, cap, window, sinks, n=H.counters())
        want = dwr.decode_window(Q, K, V, lens, h, hk, H.SCALES, chunk, cap, window, sinks)
        assert all(np.array_equal(a, w, equal_nan=True) for a, w in zip(flat(got), flat(want)))


@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("name", H.FAMILIES)
def test_the_bound_is_usable(name, d):
    """A condition: the restatement in float32 stays within half a one-flip unit of itself in float64 on every family the GPU
    file holds to FLIPS units, so FLIPS = 2 leaves the kernel its one flip and a margin."""
    worst = 0.0
    for nq, lens in H.PREFILL:
        Q, K, V = H.family(name, d, 2, 2, nq, lens)
        for b, L in enumerate(lens):
            o64, l, vmax = H.attend(Q[b][:, :d], K[b][:, :d], V[b][:, :d], L, H.SCALES)
            o32, _, _ = H.attend(Q[b][:, :d], K[b][:, :d], V[b][:, :d], L, H.SCALES, dtype=np.float32)
            assert np.isfinite(o64).all() and np.isfinite(o32).all()
            if vmax > 0:
                worst = max(worst, float((np.abs(o32 - o64) / (2.0 ** 4 * vmax / l)[:, None]).max()))
    print(f"{name} d = {d}: float32 against float64, worst {worst:.4f} units")
    assert worst <= 0.5, worst


@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("name", H.FAMILIES)
def test_the_bound_is_usable_through_the_merge_the_combine_and_the_sink(name, d):
    """The same condition on the decode restatements, streams, merge, combine and sink term all in float32: O in units of
    2^4 max|v| / Ltot, every partial in units of its own l."""
    worst = 0.0
    for h, hk, nq in H.HEADS:
        lens = H.lens_of(nq, "mid")
        Q, K, V = H.family(name, d, h, hk, nq, lens)
        for chunk, window, sinks in ((64, None, None), (128, None, None), (64, 100, H.ramp(h)), (128, 33, H.ramp(h)), (64, 1, None)):
            O, (Oc, _, pl), Ltot, vmax = H.decode(Q, K, V, lens, h, hk, H.SCALES, chunk, H.CAP, window, sinks)
            O32, (Oc32, _, pl32), _, _ = H.decode(Q, K, V, lens, h, hk, H.SCALES, chunk, H.CAP, window, sinks, dtype=np.float32)
            assert np.isfinite(O32).all() and np.array_equal(np.isnan(pl32), np.isnan(pl))
            if not vmax.any():
                continue
            worst = max(worst, float((np.abs(O32 - O) / H.o_bound(vmax, Ltot, d, 0.0, 1.0)).max()))
            w = np.repeat(~np.isnan(pl), d, axis=-1)
            if w.any():
                worst = max(worst, float((np.abs(Oc32 - Oc) / H.o_bound(vmax, np.where(np.isnan(pl) | (pl == 0), 1.0, pl), d, 0.0, 1.0))[w].max()))
    print(f"{name} d = {d}: the decode restatements in float32 against float64, worst {worst:.4f} units")
    assert worst <= 0.5, worst


def caught(fn, *args):
    try:
        fn(*args)
    except AssertionError:
        return True
    return False


def test_encode_mutants_break_the_bytes():
    t = H.edge_table()
    for scale in (1.0, 1.9):
        x = (t * np.float32(scale)).astype(np.float32)
        want = fp8_ref.encode(x, scale)
        for mutant in ("round_away", "no_clamp"):
            assert caught(H.same_bits, mutant, H.encode_mutant(x, scale, mutant), want), (mutant, scale)
    ties = H.MAGS[:-1:2].astype(np.float64) / 2 + H.MAGS[1::2] / 2  # the ties whose lower neighbour is even
    assert (H.encode_mutant(ties.astype(np.float32), 1.0, "round_away") == fp8_ref.encode(ties.astype(np.float32), 1.0) + 1).all()


def held(name, d, h, hk, nq, lens, chunk, window, sinks, mutant):
    """The GPU file's comparison of a decode call with the mutant in the kernel's place: O and the partials."""
    Q, K, V = H.family(name, d, h, hk, nq, lens)
    O, (Oc, pm, pl), Ltot, vmax = H.decode(Q, K, V, lens, h, hk, H.SCALES, chunk, H.CAP, window, sinks)
    gO, (gOc, _, _), _, _ = H.decode(Q, K, V, lens, h, hk, H.SCALES, chunk, H.CAP, window, sinks, mutant=mutant)
    fp32 = H.fp32_term(V, H.SCALES)
    if sinks is not None:  # the high sinks: the GPU file's comparison of them
        keys = H.decode(Q, K, V, lens, h, hk, H.SCALES, chunk, H.CAP, window)[2]
        H.compare_sunk(mutant, gO.astype(np.float32), (O, None, Ltot, vmax), keys, d, fp32)
    H.compare(mutant, gO.astype(np.float32), O, H.o_bound(vmax, Ltot, d, fp32))
    w = ~np.isnan(pl)
    H.compare(mutant, np.where(np.repeat(w, d, axis=-1), gOc, 0), np.where(np.repeat(w, d, axis=-1), Oc, 0), H.o_bound(vmax, np.where(w & (pl > 0), pl, 1.0), d, fp32))


MUTANTS = [  # mutant, the family that catches it, (h, h_kv, Nq), kind, chunk_rows, window, sinks
    ("mask_after_max", "superdiag", H.HEADS[0], "mid", 64, None, None),
    ("mask_after_max", "superdiag", H.HEADS[2], "edge", 128, 33, None),
    ("frozen_max", "rise", H.HEADS[0], "mid", 128, None, None),
    ("frozen_max", "spike", H.HEADS[1], "edge", 128, 100, None),
    ("merge_no_w", "oddmax", H.HEADS[1], "mid", 64, None, None),
    ("merge_no_w", "evenmax", H.HEADS[1], "mid", 64, 100, None),
    ("merge_no_w", "spike", H.HEADS[0], "edge", 64, None, None),
    ("sink_no_clamp", "rise", H.HEADS[1], "mid", 128, 33, "high"),
    ("sink_no_clamp", "rise", H.HEADS[1], "mid", 64, 100, "high"),
]


@pytest.mark.parametrize("mutant,name,hnq,kind,chunk,window,sinks", MUTANTS)
def test_mutants_of_the_decode_restatements_are_caught(mutant, name, hnq, kind, chunk, window, sinks):
    (h, hk, nq), d = hnq, 64
    lens = H.lens_of(nq, kind)
    sinks = None if sinks is None else H.high_sinks(*H.family(name, d, h, hk, nq, lens), lens, h, hk, H.CAP)
    held(name, d, h, hk, nq, lens, chunk, window, sinks, None)  # the restatement itself passes
    assert caught(held, name, d, h, hk, nq, lens, chunk, window, sinks, mutant), (mutant, name)


@pytest.mark.parametrize("mutant,name", [("mask_after_max", "superdiag"), ("frozen_max", "rise"), ("frozen_max", "spike")])
def test_mutants_of_the_prefill_restatement_are_caught(mutant, name):
    d, (nq, lens), hit = 64, H.PREFILL[0], False
    Q, K, V = H.family(name, d, 2, 2, nq, lens)
    for b, L in enumerate(lens):
        a = (Q[b][:, :d], K[b][:, :d], V[b][:, :d], L, H.SCALES)
        (O, l, vmax), (gO, _, _) = H.attend(*a), H.attend(*a, mutant=mutant)
        bound = (H.FLIPS * 2.0 ** 4 * vmax / l)[:, None] + H.fp32_term(V, H.SCALES)
        H.compare(name, O.astype(np.float32), O, bound)
        hit |= caught(H.compare, mutant, gO.astype(np.float32), O, bound)
    assert hit, (mutant, name)


def test_combine_skip_is_caught_by_a_bit_identity_only():
    """A chunk of weight below 2^-20 moves O by less than 2^-20 of it, far inside FLIPS units at any shape here:
    no bound sees this mutant.  The identity `window >= cap without sinks = attend_decode, bit for bit` does, on `rise` at the
    multi-stage shape and the GPU file's chunk_rows 192 (and at 64), where chunk weights fall through 2^-20 ... 2^-24."""
    d, (h, hk, nq), (window, chunk) = 64, H.BIG_HEADS[0], H.BIG_WINDOWS[3]
    lens = H.big_lens(nq)[1]
    Q, K, V = H.family("rise", d, h, hk, nq, lens, H.BIG_CAP)
    for c in (chunk, 64):
        want = H.decode(Q, K, V, lens, h, hk, H.SCALES, c, H.BIG_CAP)
        same = H.decode(Q, K, V, lens, h, hk, H.SCALES, c, H.BIG_CAP, window)
        skip = H.decode(Q, K, V, lens, h, hk, H.SCALES, c, H.BIG_CAP, window, mutant="combine_skip")
        H.same_bits("the windowed restatement at window >= cap", same[0].astype(np.float32), want[0].astype(np.float32))
        assert caught(H.same_bits, "combine_skip", skip[0].astype(np.float32), want[0].astype(np.float32)), c
        H.compare("combine_skip, by the bound", skip[0].astype(np.float32), want[0], H.o_bound(want[3], want[2], d, H.fp32_term(V, H.SCALES)))  # passes


def test_stage_coverage():
    """What the (lens, chunk_rows) set of the multi-stage GPU tests reaches in the decode kernels' stage loop."""
    plain = [s for _, _, nq in H.BIG_HEADS for lens in H.big_lens(nq) for L in lens for chunk in H.BIG_CHUNKS for s in [(chunk, c) for c in H.stages(L, nq, chunk)]]
    nst = {c[1] for _, c in plain}
    assert any(n >= 3 and n % 2 == 1 for n in nst) and any(n >= 4 and n % 2 == 0 for n in nst), nst  # the odd tail; a second pair
    assert {3, 4, 5, 12} <= nst
    assert any(c[1] >= 3 and c[2] == 1 for _, c in plain), "a last stage of one tile behind two full stages"
    assert any(32 * c[3] < chunk and c[1] >= 2 for chunk, c in plain), "a last chunk shorter than chunk_rows"
    assert any(chunk == 320 and c[3] == 4 for chunk, c in plain), "the 128-row last chunk of a 768-row sweep at chunk_rows 320"
    for window, chunk in H.BIG_WINDOWS:
        for _, _, nq in H.BIG_HEADS:
            NC = dwr.chunks(H.BIG_CAP, nq, window, chunk)
            assert (NC == 1) == ((window, chunk) == (128, 256))
            assert all(len(H.stages(L, nq, chunk, window)) <= NC for lens in H.big_lens(nq) for L in lens)
    direct = [c for _, _, nq in H.BIG_HEADS for lens in H.big_lens(nq) for L in lens for c in H.stages(L, nq, 256, 128)]
    assert any(t0 > 0 and n >= 3 for t0, n, _, _ in direct), "the one-launch form: t0 > 0 and three stages"
    wide = [c for _, _, nq in H.BIG_HEADS for lens in H.big_lens(nq) for L in lens for c in H.stages(L, nq, 192, 500)]
    assert any(t0 > 0 and n == 3 for t0, n, _, _ in wide) and any(t0 > 0 and last == 1 for t0, _, last, _ in wide)
    # a page of more than one stage, entered in its middle: a chunk that starts inside a page
    assert any((chunk // 64 * c) % (page // 64) != 0 for chunk in H.BIG_CHUNKS for page in H.BIG_PAGES for c in range(1, H.BIG_CAP // chunk))
