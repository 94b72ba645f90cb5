"""Re-entrancy of the drop-in boundary (the reference's `solve` is re-entrant in practice --
per-call cudaMalloc'd scratch and private streams, include/launchers.h:27-33,64-71).

The library caches its scratch per (device, stream) instead, and a call holds a lease on that slot from the
moment the buffer is handed out until its last kernel is enqueued (qmha_api.cpp, lease_workspace).  These
tests run concurrent host threads through every C-ABI entry a binding uses -- the per-variant `solve` of
libqmha_fa_tc_int8_b.so (blocking, null stream), qmha_solve_ex on one SHARED stream, and the ctypes
jax_ext.flash_solve (blocking, which releases the GIL like the torch ctypes front-end) -- with different
inputs and growing problem sizes (so the slot's buffer is retired and reallocated while other threads'
work is in flight), and require every output to be bit-identical to the same call made single-threaded.

And the scratch contents never matter: qmha_solve_ws on a caller workspace full of random bytes, or left
holding another input set's intermediates, gives the library call's output bit for bit."""
import ctypes
import os
import threading

import pytest

from tests.gpu_support import dev, overlap_chunks  # noqa: F401

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


THREADS, CALLS = 4, 25
H, D = 4, 64
VARIANTS = ("fa_tc_int8_b", "fa_tc_int8_pt", "fa_tc_v1a")
ENTRIES = ("solve", "solve_ex", "jax")


def _plan(t, j):
    """(entry, variant, B, N) of call j of thread t: every entry point and variant in every thread, and N
    growing over the run (the largest size of each thread first appears at call >= 9, so its slot grows
    while the other threads' work is in flight)."""
    entry = ENTRIES[(j + t) % 3]
    variant = "fa_tc_int8_b" if entry == "solve" else VARIANTS[(j + 2 * t) % 3]
    B = 2 if entry == "solve_ex" else 1
    N = (128, 256, 96, 512, 160, 1024, 384)[min(j // 3, 6) if j % 4 else (j + t) % 4]
    return entry, variant, B, N


def test_concurrent_callers_bit_identical(dev):
    from quantizedmha_amd import _lib, jax_ext
    lib = _lib.load()
    solve_lib = ctypes.CDLL(os.path.join(ROOT, "quantizedmha_amd", "lib", "libqmha_fa_tc_int8_b.so"))
    solve_lib.solve.restype = None
    solve_lib.solve.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_int] * 3
    shared = torch.cuda.Stream(dev)
    sptr = shared.cuda_stream
    calls = {}
    for t in range(THREADS):
        for j in range(CALLS):
            entry, variant, B, N = _plan(t, j)
            g = torch.Generator(device=dev).manual_seed(1000 * t + j)
            Q, K, V = (torch.randn(B, N, H * D, device=dev, generator=g) * (0.4 + 0.05 * j) for _ in range(3))
            calls[t, j] = (entry, variant, B, N, Q, K, V, torch.full_like(Q, float("nan")))
    # single-threaded references: the same variant on the same inputs, one call at a time
    refs = {}
    for key, (entry, variant, B, N, Q, K, V, _) in calls.items():
        R = torch.empty_like(Q)
        _lib.check(lib.qmha_solve_ex(Q.data_ptr(), K.data_ptr(), V.data_ptr(), R.data_ptr(), B, N, H * D, H,
                                     _lib.variant_id(variant), None))
        torch.cuda.synchronize(dev)
        refs[key] = R
    lib.qmha_release_workspaces()  # every slot starts empty: the threads' calls grow them
    torch.cuda.synchronize(dev)
    errors = []
    start = threading.Barrier(THREADS)

    def worker(t):
        try:
            torch.cuda.set_device(dev)
            start.wait()
            for j in range(CALLS):
                entry, variant, B, N, Q, K, V, O = calls[t, j]
                if entry == "solve":  # blocking, null stream (reference launchers.h:64)
                    solve_lib.solve(Q.data_ptr(), K.data_ptr(), V.data_ptr(), O.data_ptr(), N, H * D, H)
                elif entry == "solve_ex":  # asynchronous, one stream shared by all threads
                    _lib.check(lib.qmha_solve_ex(Q.data_ptr(), K.data_ptr(), V.data_ptr(), O.data_ptr(), B, N, H * D,
                                                 H, _lib.variant_id(variant), sptr))
                else:  # the ctypes raw-pointer binding (extensions/jax/jax_ext.cpp), blocking
                    jax_ext.flash_solve(Q.data_ptr(), K.data_ptr(), V.data_ptr(), O.data_ptr(), N, H * D, H, variant)
        except Exception as e:  # reported below; the other threads go on
            errors.append(f"thread {t}: {e!r}")

    threads = [threading.Thread(target=worker, args=(t,)) for t in range(THREADS)]
    for th in threads:
        th.start()
    for th in threads:
        th.join(timeout=90)
    assert not any(th.is_alive() for th in threads), "a caller thread hung"
    shared.synchronize()
    torch.cuda.synchronize(dev)
    assert not errors, errors
    bad = []
    for key, (entry, variant, B, N, Q, K, V, O) in calls.items():
        if not torch.equal(O, refs[key]):
            d = (O - refs[key]).abs().nan_to_num(1e30).max().item()
            bad.append(f"thread {key[0]} call {key[1]} {entry} {variant} B{B} N{N}: max|diff| {d:.3g}")
    assert not bad, f"{len(bad)} of {len(calls)} calls differ from their single-threaded result: " + "; ".join(bad[:8])
    seen = {(c[0], c[1]) for c in calls.values()}
    assert {e for e, _ in seen} == set(ENTRIES) and {v for _, v in seen} == set(VARIANTS), seen


@pytest.mark.parametrize("variant,B,N,d", [("fa_tc_int8_b", 3, 1024, 64), ("fa_tc_int8_b", 2, 96, 32),
                                           ("fa_tc_int8_pt", 3, 1024, 64), ("fa_tc_int8_pt", 2, 512, 128),
                                           ("fa_tc_v1a", 3, 1024, 64), ("fa_tc_int8_b", 1, 256, 96)])
def test_scratch_contents_never_matter(dev, variant, B, N, d):
    """qmha_solve_ws on a caller workspace of random bytes, then back-to-back calls of three input sets on it
    without refilling (each call's scratch holds the previous set's intermediates): every output equals the
    library call's bit for bit."""
    from quantizedmha_amd import _lib
    lib = _lib.load()
    vid = _lib.variant_id(variant)
    Hh = 4
    dm = Hh * d
    stream = torch.cuda.current_stream(dev).cuda_stream
    g = torch.Generator(device=dev).manual_seed(31 + N + B + d)
    sets = [tuple(torch.randn(B, N, dm, device=dev, generator=g) * (0.5 + 0.25 * i) for _ in range(3)) for i in range(3)]

    def call(i, ws=None):
        Q, K, V = sets[i]
        O = torch.full_like(Q, float("nan"))
        if ws is None:
            _lib.check(lib.qmha_solve_ex(Q.data_ptr(), K.data_ptr(), V.data_ptr(), O.data_ptr(), B, N, dm, Hh, vid, stream))
        else:
            _lib.check(lib.qmha_solve_ws(Q.data_ptr(), K.data_ptr(), V.data_ptr(), O.data_ptr(), B, N, dm, Hh, vid,
                                         ws.data_ptr(), ws.numel(), stream))
        torch.cuda.synchronize(dev)
        return O

    refs = [call(i) for i in range(3)]
    for r in refs:
        assert torch.isfinite(r).all()
    ws = torch.empty(lib.qmha_workspace_size(B, N, dm, Hh, vid), dtype=torch.uint8, device=dev)
    for i in range(3):
        ws.random_(0, 256)
        assert torch.equal(call(i, ws), refs[i]), f"poisoned workspace, set {i}"
    for i in (2, 0, 1, 2):
        assert torch.equal(call(i, ws), refs[i]), f"back-to-back, set {i}"
    assert not torch.equal(refs[0], refs[1])


# ---- one leased slot per (device, stream): every solve entry, the overlap side stream, release ----------
H2, D2 = 2, 64
CAUSAL_VARIANTS = ("fa_tc_int8_b", "fa_tc_v1a")  # the chunked variants; fa_tc_int8_pt is the unchunked branch


def _hip_stream_per_thread():
    """The hipStreamPerThread handle as the installed ROCm's hip_runtime_api.h defines it."""
    import re
    header = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include", "hip", "hip_runtime_api.h")
    m = re.search(r"#define\s+hipStreamPerThread\s+\(\(hipStream_t\)\s*(\w+)\)", open(header).read())
    assert m, header
    return int(m.group(1), 0)


def _make_calls(dev, plan):
    """plan: {key: (entry, variant, B, N)} -> {key: (entry, variant, B, N, Q, K, V, O)}, O filled with NaN."""
    calls = {}
    for i, (key, (entry, variant, B, N)) in enumerate(sorted(plan.items())):
        g = torch.Generator(device=dev).manual_seed(7000 + i)
        Q, K, V = (torch.randn(B, N, H2 * D2, device=dev, generator=g) * (0.4 + 0.03 * i) for _ in range(3))
        calls[key] = (entry, variant, B, N, Q, K, V, torch.full_like(Q, float("nan")))
    return calls


def _enqueue(lib, call, O, stream, ws=None):
    """One call through its entry point: "ex" qmha_solve_ex, "ws" qmha_solve_ws on the caller workspace `ws`,
    "causal" qmha_solve_opts with QMHA_FLAG_CAUSAL and a null workspace."""
    from quantizedmha_amd import _lib
    entry, variant, B, N, Q, K, V, _ = call
    args = (Q.data_ptr(), K.data_ptr(), V.data_ptr(), O.data_ptr(), B, N, H2 * D2, H2, _lib.variant_id(variant))
    if entry == "ex":
        st = lib.qmha_solve_ex(*args, stream)
    elif entry == "ws":
        st = lib.qmha_solve_ws(*args, ws.data_ptr(), ws.numel(), stream)
    else:
        st = lib.qmha_solve_opts(*args, _lib.QMHA_FLAG_CAUSAL, None, 0, stream)
    _lib.check(st, f"{entry} {variant} B{B} N{N}")


def _ws_bytes(lib, call):
    from quantizedmha_amd import _lib
    _, variant, B, N = call[:4]
    return lib.qmha_workspace_size(B, N, H2 * D2, H2, _lib.variant_id(variant))


def _references(dev, lib, calls, stream_of):
    """The same calls made one at a time with overlap chunks = 1."""
    ws = torch.empty(max(max(_ws_bytes(lib, c) for c in calls.values()), 256), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)  # the inputs were made on the default stream
    refs = {}
    with overlap_chunks(1):
        for key, call in calls.items():
            refs[key] = torch.full_like(call[4], float("nan"))
            _enqueue(lib, call, refs[key], stream_of(key), ws)
            torch.cuda.synchronize(dev)
    return refs


def _run_threads(dev, workers):
    """Start every worker(errors) at once, join with a timeout; returns the errors the workers reported."""
    errors = []
    start = threading.Barrier(len(workers))

    def body(i, fn):
        try:
            torch.cuda.set_device(dev)
            start.wait()
            fn()
        except Exception as e:  # reported below; the other threads go on
            errors.append(f"thread {i}: {e!r}")

    threads = [threading.Thread(target=body, args=(i, fn)) for i, fn in enumerate(workers)]
    for th in threads:
        th.start()
    for th in threads:
        th.join(timeout=60)
    assert not any(th.is_alive() for th in threads), "a thread hung"
    return errors


def _assert_bit_identical(calls, refs):
    bad = []
    for key, (entry, variant, B, N, Q, K, V, O) in calls.items():
        assert torch.isfinite(refs[key]).all(), key
        if not torch.equal(O, refs[key]):
            d = (O - refs[key]).abs().nan_to_num(1e30).max().item()
            bad.append(f"{key} {entry} {variant} B{B} N{N}: max|diff| {d:.3g}")
    assert not bad, f"{len(bad)} of {len(calls)} calls differ from their single-threaded result: " + "; ".join(bad[:8])


def test_concurrent_callers_with_overlap_chunks(dev):
    """4 threads x 9 calls on one shared stream with overlap chunks = 2 (the slot's side stream in use), through
    qmha_solve_ex, qmha_solve_ws (one caller workspace per thread: it leases the slot too) and causal
    qmha_solve_opts; B = 3 is the uneven 1 + 2 chunk split, N = 96 ends on a partial stage."""
    from quantizedmha_amd import _lib
    lib = _lib.load()
    nthreads, ncalls = 4, 9
    plan = {}
    for t in range(nthreads):
        for j in range(ncalls):
            entry = ("ex", "ws", "causal")[(j + t) % 3]  # each entry once per block of three calls ...
            pool = CAUSAL_VARIANTS if entry == "causal" else VARIANTS
            variant = pool[(j // 3 + t) % len(pool)]  # ... with another variant in every block
            plan[t, j] = (entry, variant, 2 + (j + j // 3) % 2, (96, 128, 256)[(j + t + j // 3) % 3])
    seen = set(plan.values())
    assert {(e, v) for e, v, _, _ in seen} == {(e, v) for e in ("ex", "ws") for v in VARIANTS} | \
        {("causal", v) for v in CAUSAL_VARIANTS}
    assert {b for _, _, b, _ in seen} == {2, 3} and {n for _, _, _, n in seen} == {96, 128, 256}
    calls = _make_calls(dev, plan)
    shared = torch.cuda.Stream(dev)
    sptr = shared.cuda_stream
    refs = _references(dev, lib, calls, lambda key: sptr)
    wss = [torch.empty(max(_ws_bytes(lib, c) for (t2, _), c in calls.items() if t2 == t and c[0] == "ws"),
                       dtype=torch.uint8, device=dev) for t in range(nthreads)]
    torch.cuda.synchronize(dev)  # inputs, references and workspaces exist before the threads start

    def worker(t):
        def fn():
            for j in range(ncalls):
                _enqueue(lib, calls[t, j], calls[t, j][7], sptr, wss[t])
        return fn

    with overlap_chunks(2):
        errors = _run_threads(dev, [worker(t) for t in range(nthreads)])
        shared.synchronize()
        torch.cuda.synchronize(dev)
    assert not errors, errors
    _assert_bit_identical(calls, refs)


def test_release_beside_callers_with_overlap_chunks(dev):
    """qmha_release_workspaces is safe beside running callers, overlap chunks > 1 included
    (the side stream and its events live in the leased slot).  3 threads x 10 qmha_solve_ex calls, two on a
    shared stream and one on its own, while a fourth thread releases five times about 20 ms apart: no call
    fails and every output is bit-identical to its single-threaded, chunks = 1 result."""
    import time
    from quantizedmha_amd import _lib
    lib = _lib.load()
    ncallers, ncalls = 3, 10
    plan = {(t, j): ("ex", CAUSAL_VARIANTS[(j + t) % 2], 2, (96, 256)[(j // 2 + t) % 2])
            for t in range(ncallers) for j in range(ncalls)}
    calls = _make_calls(dev, plan)
    streams = [torch.cuda.Stream(dev), torch.cuda.Stream(dev)]
    sptr = lambda key: streams[key[0] // 2].cuda_stream  # noqa: E731  threads 0, 1 share; thread 2 has its own
    refs = _references(dev, lib, calls, sptr)
    torch.cuda.synchronize(dev)

    def caller(t):
        def fn():
            for j in range(ncalls):
                _enqueue(lib, calls[t, j], calls[t, j][7], sptr((t, j)))
        return fn

    def releaser():
        for _ in range(5):
            lib.qmha_release_workspaces()
            time.sleep(0.02)

    with overlap_chunks(2):
        errors = _run_threads(dev, [caller(t) for t in range(ncallers)] + [releaser])
        torch.cuda.synchronize(dev)
    assert not errors, errors
    _assert_bit_identical(calls, refs)


def test_stream_per_thread_slots(dev):
    """hipStreamPerThread names another stream in every thread, so every thread has a slot of its own (scratch
    and side stream): 3 threads x 6 qmha_solve_ex calls on that handle with sizes growing 96 -> 256 -> 512
    within each thread (each slot grows), overlap chunks = 2."""
    from quantizedmha_amd import _lib
    lib = _lib.load()
    per_thread = _hip_stream_per_thread()
    nthreads, ncalls = 3, 6
    plan = {(t, j): ("ex", VARIANTS[(j + t) % 3], 2, (96, 256, 512)[j // 2]) for t in range(nthreads) for j in range(ncalls)}
    calls = _make_calls(dev, plan)
    refs = _references(dev, lib, calls, lambda key: per_thread)
    torch.cuda.synchronize(dev)

    def worker(t):
        def fn():
            for j in range(ncalls):
                _enqueue(lib, calls[t, j], calls[t, j][7], per_thread)
        return fn

    with overlap_chunks(2):
        errors = _run_threads(dev, [worker(t) for t in range(nthreads)])
        torch.cuda.synchronize(dev)  # device-wide: the per-thread streams are not reachable from here
    assert not errors, errors
    _assert_bit_identical(calls, refs)
