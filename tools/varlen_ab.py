#!/usr/bin/env python3
"""Per-sequence lengths read on the device (qmha_attend_cached_varlen) against the uniform
qmha_attend_cached, in one process, alternating.

    python tools/varlen_ab.py --variant fa_tc_int8_b --B 16 --H 16 --d 64 --cap 4096

A cache of `cap` rows is filled once.  With qmha_profile on, both sides of a case are warmed, then ROUNDS rounds
alternate CALLS reference and CALLS candidate calls; the figures are the library's own main-kernel event pairs and a
device-event pair around each batch (the whole call, launches included).  One JSON line per case:
  a  every lens[b] == cap, at Nq = 1024 and Nq = 32, against qmha_attend_cached at len == cap: what the per-sequence
     scalars cost.  Expected: main_ratio 1 within the reference's own round-to-round spread (ref_main_spread =
     (max - min) / median of its rounds).
  b  lens spread evenly over 512 .. cap, decode (Nq = 32), against qmha_attend_cached at len == cap: main_ratio beside
     the visited-tile ratio R = mean(lens) / cap and the project's bound 1.2 R.
  c  the same lens against what the library offered before: B caches of one sequence each, holding lens[b] rows, and B
     qmha_attend_cached launches.  main_ratio: one varlen kernel over the sum of the B kernels; call_ratio: the whole
     step, launches included.
The candidate's O is compared with the reference's bit for bit before anything is timed (case b: with case c's).
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
    ap.add_argument("--prefill", type=int, default=1024, help="case a's long Nq")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    if a.rounds < 5 or a.calls < 30:
        ap.error("at least 5 rounds of at least 30 calls")
    if a.cap % 32 or a.cap < 1024 or a.prefill % 32 or not 32 <= a.prefill <= a.cap or a.B < 2:
        ap.error("cap % 32 == 0, cap >= 1024, 32 <= prefill <= cap, B >= 2")

    import torch
    import bench
    from quantizedmha_amd import _lib, isa_id, torch_ext
    lib = _lib.load()
    dev = torch.device("cuda:0")
    dm = a.H * a.d
    g = torch.Generator(device=dev).manual_seed(a.cap + a.d)
    K, V = (torch.rand((a.B, a.cap, dm), generator=g, device=dev, dtype=torch.float32) for _ in range(2))
    Q = torch.rand((a.B, a.prefill, dm), generator=g, device=dev, dtype=torch.float32)
    stream = torch.cuda.current_stream(dev).cuda_stream
    stem = "int8" if a.variant == "fa_tc_int8_b" else "f16"
    CAUSAL = _lib.QMHA_FLAG_CAUSAL

    cache = torch_ext.KVCache(a.B, a.cap, dm, a.H, a.variant, device=dev)
    cache.append(K, V)
    # lens evenly over 512 .. cap, in whole tiles
    t0, t1 = 512 // 32, a.cap // 32
    spread = [32 * (t0 + round(i * (t1 - t0) / (a.B - 1))) for i in range(a.B)]
    singles = []  # case c: one cache per sequence, holding its lens[b] rows
    for b, L in enumerate(spread):
        c = torch_ext.KVCache(1, a.cap, dm, a.H, a.variant, device=dev)
        c.append(K[b:b + 1, :L].contiguous(), V[b:b + 1, :L].contiguous())
        singles.append(c)

    def uniform(q, o):
        return lambda: _lib.check(lib.qmha_attend_cached(cache._handle, q.data_ptr(), o.data_ptr(), q.shape[1], CAUSAL, stream),
                                  "attend")

    def varlen(q, o, lens):
        return lambda: _lib.check(lib.qmha_attend_cached_varlen(cache._handle, q.data_ptr(), o.data_ptr(), q.shape[1],
                                                                lens.data_ptr(), CAUSAL, stream), "attend_varlen")

    def one_by_one(q, o):
        def call():
            for b, c in enumerate(singles):
                _lib.check(lib.qmha_attend_cached(c._handle, q[b].data_ptr(), o[b].data_ptr(), q.shape[1], CAUSAL, stream),
                           "attend")
        return call

    def batch(call, n, records):
        """n calls: (main-kernel ms per call, whole-call ms per call)."""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            call()
        e1.record()
        torch.cuda.synchronize(dev)
        main_ms, pre_ms, k = ctypes.c_double(), ctypes.c_double(), ctypes.c_longlong()
        _lib.check(lib.qmha_profile_collect(ctypes.byref(main_ms), ctypes.byref(k), ctypes.byref(pre_ms)), "collect")
        assert k.value == records * n, (k.value, records, n)
        return main_ms.value / n, e0.elapsed_time(e1) / n

    def measure(sides):
        """sides: {name: (call, records per call)}, reference first.  Per-round rows and medians per side."""
        lib.qmha_profile_collect(None, None, None)
        lib.qmha_profile_enable(1)
        try:
            for call, rec in sides.values():
                batch(call, a.warmup, rec)
            rows = {s: [] for s in sides}
            for _ in range(a.rounds):
                for s, (call, rec) in sides.items():
                    rows[s].append(batch(call, a.calls, rec))
        finally:
            lib.qmha_profile_enable(0)
        med = {s: [statistics.median(r[i] for r in rows[s]) for i in range(2)] for s in rows}
        return rows, med

    def report(case, Nq, ref, cand, rows, med, extra):
        ref_main = [r[0] for r in rows[ref]]
        res = {"tool": "varlen_ab", "case": case, "variant": a.variant, "B": a.B, "H": a.H, "d": a.d, "cap": a.cap, "Nq": Nq,
               "rounds": a.rounds, "calls_per_round": a.calls, "reference": ref,
               "ref_main_kernel_ms": round(med[ref][0], 5), "varlen_main_kernel_ms": round(med[cand][0], 5),
               "ref_call_ms": round(med[ref][1], 5), "varlen_call_ms": round(med[cand][1], 5),
               "main_ratio": round(med[cand][0] / med[ref][0], 4),
               "ref_main_spread": round((max(ref_main) - min(ref_main)) / med[ref][0], 4),
               "call_ratio": round(med[cand][1] / med[ref][1], 4)}
        res.update(extra)
        res.update({"per_round": {s: [[round(x, 5) for x in r] for r in rows[s]] for s in rows},
                    "clock_probe": bench.clock_probe(dev),
                    "isa_sha16": {"uniform_main": isa_id.isa_sha16(_lib.LIB_PATH, f"qmha_fa_{stem}_masked_kernelILi{a.d}ENS_4RectE"),
                                  "varlen_main": isa_id.isa_sha16(_lib.LIB_PATH, f"qmha_fa_{stem}_varlen_kernelILi{a.d}E")},
                    "device": torch.cuda.get_device_properties(dev).name})
        print(json.dumps(res), flush=True)

    # ---- a: every length == cap -------------------------------------------------------------------------------
    full = torch.full((a.B,), a.cap, dtype=torch.int32, device=dev)
    for Nq in (a.prefill, 32):
        q = Q[:, :Nq].contiguous()
        o_ref, o_var = torch.empty_like(q), torch.empty_like(q)
        sides = {"uniform": (uniform(q, o_ref), 1), "varlen": (varlen(q, o_var, full), 1)}
        for call, _ in sides.values():
            call()
        torch.cuda.synchronize(dev)
        same = bool(torch.equal(o_ref, o_var))
        rows, med = measure(sides)
        report("a", Nq, "uniform", "varlen", rows, med, {"lens": "all cap", "bit_identical": same})

    # ---- b, c: lengths spread over 512 .. cap, decode ---------------------------------------------------------
    lens = torch.tensor(spread, dtype=torch.int32, device=dev)
    q = Q[:, :32].contiguous()
    o_uni, o_var, o_one = torch.empty_like(q), torch.empty_like(q), torch.empty_like(q)
    sides = {"uniform": (uniform(q, o_uni), 1), "varlen": (varlen(q, o_var, lens), 1), "one_by_one": (one_by_one(q, o_one), a.B)}
    for call, _ in sides.values():
        call()
    torch.cuda.synchronize(dev)
    same = bool(torch.equal(o_one, o_var))
    R = sum(spread) / (a.B * a.cap)
    rows, med = measure(sides)
    ratio = med["varlen"][0] / med["uniform"][0]
    report("b", 32, "uniform", "varlen", rows, med,
           {"lens": spread, "bit_identical_to_one_by_one": same, "visited_tile_ratio_R": round(R, 4), "bound_1.2R": round(1.2 * R, 4),
            "within_bound": bool(ratio <= 1.2 * R)})
    report("c", 32, "one_by_one", "varlen", rows, med,
           {"lens": spread, "bit_identical": same, "reference_launches": a.B})


if __name__ == "__main__":
    main()
