#!/usr/bin/env python3
"""A decode step at ragged lengths (qmha_kv_cache_append_tokens n = 1 plus qmha_attend_cached_tokens Nq = 1)
against the step the library offered before at the next multiple of 32 (qmha_kv_cache_append_at n = 32 plus
qmha_attend_cached_varlen Nq = 32), in one process, alternating.

    python tools/tokens_ab.py --variant fa_tc_int8_b --B 16 --H 16 --d 64 --cap 4096

Two caches of `cap` rows are filled once.  Sequence b holds L[b] = 32 t[b] + r rows, t[b] spread evenly over 512 / 32 ..
cap / 32 - 1 and r = 17 for all (one n per call): the candidate's open group is built by append_tokens from its first
row on, so its tail is what a serving loop would hold.  The candidate step appends row L[b] - 1 again and attends
with one query row; the reference step places the 32 rows of group t[b] and attends with 32 query rows at
32 (t[b] + 1).  Both visit t[b] + 1 key tiles per head with one active query group, so the main-kernel ratio is
expected near 1.  With qmha_profile on, both sides are warmed, then ROUNDS rounds alternate CALLS reference and CALLS
candidate steps; the figures are the library's own event pairs (append: pre-pass, attend: main kernel) and a
device-event pair around each batch (the whole step, launches included).  One JSON line.
The candidate's O is compared bit for bit, before anything is timed, with the padded path the contract names: rows
r - 1 of attend_varlen on a zero 32-row block holding q there, at 32 (t[b] + 1), over the candidate's cache.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variant", default="fa_tc_int8_b", choices=["fa_tc_int8_b", "fa_tc_v1a"])
    ap.add_argument("--B", type=int, default=16)
    ap.add_argument("--H", type=int, default=16)
    ap.add_argument("--d", type=int, default=64)
    ap.add_argument("--cap", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    if a.rounds < 5 or a.calls < 30:
        ap.error("at least 5 rounds of at least 30 calls")
    if a.cap % 32 or a.cap < 1024 or a.B < 2:
        ap.error("cap % 32 == 0, cap >= 1024, B >= 2")

    import torch
    import bench
    from quantizedmha_amd import _lib, isa_id, torch_ext
    lib = _lib.load()
    dev = torch.device("cuda:0")
    dm, r = a.H * a.d, 17
    g = torch.Generator(device=dev).manual_seed(a.cap + a.d)
    K, V = (torch.rand((a.B, a.cap, dm), generator=g, device=dev, dtype=torch.float32) for _ in range(2))
    Q = torch.rand((a.B, 32, dm), generator=g, device=dev, dtype=torch.float32)
    stream = torch.cuda.current_stream(dev).cuda_stream
    stem = "int8" if a.variant == "fa_tc_int8_b" else "f16"
    CAUSAL = _lib.QMHA_FLAG_CAUSAL
    i32 = lambda xs: torch.tensor(xs, dtype=torch.int32, device=dev)  # noqa: E731

    t0, t1 = 512 // 32, a.cap // 32 - 1
    tiles = [t0 + round(i * (t1 - t0) / (a.B - 1)) for i in range(a.B)]
    L = [32 * t + r for t in tiles]
    rows = lambda X, first, n: torch.stack([X[b, p:p + n] for b, p in enumerate(first)]).contiguous()  # noqa: E731

    cand, ref = (torch_ext.KVCache(a.B, a.cap, dm, a.H, a.variant, device=dev) for _ in range(2))
    for c in (cand, ref):
        c.append(K, V)
    cand.enable_tokens()
    base = [32 * t for t in tiles]
    cand.append_tokens(rows(K, base, r - 1), rows(V, base, r - 1), i32(base))  # the open group, from its first row on

    k1, v1, q1 = rows(K, [x - 1 for x in L], 1), rows(V, [x - 1 for x in L], 1), Q[:, r - 1:r].contiguous()
    k32, v32, q32 = rows(K, base, 32), rows(V, base, 32), Q
    pos1, lens1, pos32, lens32 = i32([x - 1 for x in L]), i32(L), i32(base), i32([x + 32 for x in base])
    o1, o32 = torch.empty_like(q1), torch.empty_like(q32)

    def tokens_step():
        _lib.check(lib.qmha_kv_cache_append_tokens(cand._handle, k1.data_ptr(), v1.data_ptr(), 1, pos1.data_ptr(), stream), "append_tokens")
        _lib.check(lib.qmha_attend_cached_tokens(cand._handle, q1.data_ptr(), o1.data_ptr(), 1, lens1.data_ptr(), CAUSAL, stream),
                   "attend_tokens")

    def padded_step():
        _lib.check(lib.qmha_kv_cache_append_at(ref._handle, k32.data_ptr(), v32.data_ptr(), 32, pos32.data_ptr(), stream), "append_at")
        _lib.check(lib.qmha_attend_cached_varlen(ref._handle, q32.data_ptr(), o32.data_ptr(), 32, lens32.data_ptr(), CAUSAL, stream),
                   "attend_varlen")

    # O before timing: the candidate against the padded path over its own cache
    tokens_step()
    qp = torch.zeros_like(Q)
    qp[:, r - 1] = q1[:, 0]
    want = cand.attend_varlen(qp, lens32)[:, r - 1:r]
    torch.cuda.synchronize(dev)
    same = bool(torch.equal(o1, want)) and bool(torch.isfinite(o1).all()) and float(o1.abs().max()) > 0.0

    def batch(call, n):
        """n steps: (main-kernel ms, pre-pass ms, whole-step ms) per step."""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            call()
        e1.record()
        torch.cuda.synchronize(dev)
        main_ms, pre_ms, k = ctypes.c_double(), ctypes.c_double(), ctypes.c_longlong()
        _lib.check(lib.qmha_profile_collect(ctypes.byref(main_ms), ctypes.byref(k), ctypes.byref(pre_ms)), "collect")
        assert k.value == 2 * n, (k.value, n)  # one record per append, one per attend
        return main_ms.value / n, pre_ms.value / n, e0.elapsed_time(e1) / n

    sides = {"padded": padded_step, "tokens": tokens_step}  # the reference first
    lib.qmha_profile_collect(None, None, None)
    lib.qmha_profile_enable(1)
    try:
        for call in sides.values():
            batch(call, a.warmup)
        per = {s: [] for s in sides}
        for _ in range(a.rounds):
            for s, call in sides.items():
                per[s].append(batch(call, a.calls))
    finally:
        lib.qmha_profile_enable(0)
    med = {s: [statistics.median(x[i] for x in per[s]) for i in range(3)] for s in per}
    ref_main = [x[0] for x in per["padded"]]
    res = {"tool": "tokens_ab", "variant": a.variant, "B": a.B, "H": a.H, "d": a.d, "cap": a.cap, "lens": L,
           "rounds": a.rounds, "calls_per_round": a.calls, "reference": "append_at n=32 + attend_varlen Nq=32 at ceil32(L)",
           "candidate": "append_tokens n=1 + attend_tokens Nq=1 at L", "bit_identical_to_padded_path": same,
           "ref_main_kernel_ms": round(med["padded"][0], 5), "tokens_main_kernel_ms": round(med["tokens"][0], 5),
           "ref_append_ms": round(med["padded"][1], 5), "tokens_append_ms": round(med["tokens"][1], 5),
           "ref_step_ms": round(med["padded"][2], 5), "tokens_step_ms": round(med["tokens"][2], 5),
           "main_ratio": round(med["tokens"][0] / med["padded"][0], 4),
           "ref_main_spread": round((max(ref_main) - min(ref_main)) / med["padded"][0], 4),
           "append_ratio": round(med["tokens"][1] / med["padded"][1], 4),
           "step_ratio": round(med["tokens"][2] / med["padded"][2], 4),
           "per_round": {s: [[round(x, 5) for x in row] for row in per[s]] for s in per},
           "clock_probe": bench.clock_probe(dev),
           "isa_sha16": {"varlen_main": isa_id.isa_sha16(_lib.LIB_PATH, f"qmha_fa_{stem}_varlen_kernelILi{a.d}E"),
                         "ragged_main": isa_id.isa_sha16(_lib.LIB_PATH, f"qmha_fa_{stem}_cache_kernelILi{a.d}ENS_6RaggedEEEv")},
           "device": torch.cuda.get_device_properties(dev).name}
    print(json.dumps(res), flush=True)
    if not same:
        sys.exit("tokens_ab: the candidate's O is not the padded path's")


if __name__ == "__main__":
    main()
