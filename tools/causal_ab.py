#!/usr/bin/env python3
"""Causal against non-causal attention at one shape, in one process, alternating.

    python tools/causal_ab.py --variant fa_tc_int8_b --B 16 --H 16 --N 4096 --d 64

The reference time is the shipped non-causal main kernel, measured on the same device in the same
minute.  With qmha_profile on, both paths are warmed, then ROUNDS rounds alternate CALLS non-causal and
CALLS causal calls; the medians over the rounds of the per-call main-kernel time (the library's own
event pairs) and of the whole-call time (events around the batch of calls) are printed as one JSON line with
their ratio.  The expected ratio is the workgroup-level tile ratio
    R = sum_qb min(G, WAVES (qb + 1)) / (nqb G),   G = N / 32, nqb = ceil(G / WAVES)
with the causal kernels' WAVES query groups per workgroup (a workgroup's KV loop runs to its last wave's
diagonal tile); DESIGN.md 10 holds the measured ratio to 1.2 R.
"""
import argparse
import ctypes
import json
import os
import re
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# the shipped query groups per workgroup, read from the kernel source
with open(os.path.join(ROOT, "quantizedmha_amd", "csrc", "qmha_fa_masked.hpp")) as _f:
    CAUSAL_WAVES = int(re.search(r"constexpr int kWaves = (\d+)", _f.read()).group(1))


def tile_ratio(N, waves=CAUSAL_WAVES):
    G = N // 32
    nqb = (G + waves - 1) // waves
    return sum(min(G, waves * (qb + 1)) for qb in range(nqb)) / (nqb * G)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variant", default="fa_tc_int8_b", choices=["fa_tc_int8_b", "fa_tc_v1a"])
    ap.add_argument("--B", type=int, default=16)
    ap.add_argument("--H", type=int, default=16)
    ap.add_argument("--N", type=int, default=4096)
    ap.add_argument("--d", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    if a.rounds < 5 or a.calls < 30:
        ap.error("at least 5 rounds of at least 30 calls")

    import torch
    import bench
    from quantizedmha_amd import _lib, isa_id
    lib = _lib.load()
    dev = torch.device("cuda:0")
    dm = a.H * a.d
    g = torch.Generator(device=dev).manual_seed(a.N + a.d)
    Q, K, V = (torch.rand((a.B, a.N, dm), generator=g, device=dev, dtype=torch.float32) for _ in range(3))
    O = torch.empty_like(Q)
    vid = _lib.VARIANTS[a.variant]
    stream = torch.cuda.current_stream(dev).cuda_stream

    def call(flags):
        _lib.check(lib.qmha_solve_opts(Q.data_ptr(), K.data_ptr(), V.data_ptr(), O.data_ptr(), a.B, a.N, dm, a.H, vid,
                                       flags, None, 0, stream), "causal_ab")

    def batch(flags, n):
        """n calls: (main-kernel ms per call, pre-pass ms per call, whole-call ms per call)."""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            call(flags)
        e1.record()
        torch.cuda.synchronize(dev)
        main_ms, pre_ms, k = ctypes.c_double(), ctypes.c_double(), ctypes.c_longlong()
        _lib.check(lib.qmha_profile_collect(ctypes.byref(main_ms), ctypes.byref(k), ctypes.byref(pre_ms)), "collect")
        assert k.value == n, (k.value, n)
        return main_ms.value / n, pre_ms.value / n, e0.elapsed_time(e1) / n

    lib.qmha_profile_collect(None, None, None)
    lib.qmha_profile_enable(1)
    try:
        for flags in (0, _lib.QMHA_FLAG_CAUSAL):
            batch(flags, a.warmup)
        rows = {0: [], 1: []}
        for _ in range(a.rounds):
            for flags in (0, _lib.QMHA_FLAG_CAUSAL):
                rows[flags].append(batch(flags, a.calls))
    finally:
        lib.qmha_profile_enable(0)
    med = {f: [statistics.median(r[i] for r in rows[f]) for i in range(3)] for f in rows}
    R = tile_ratio(a.N)
    ratio = med[1][0] / med[0][0]
    ids = bench.isa_ids(a.variant, a.d)
    ckern = "qmha_fa_%s_masked_kernelILi%dENS_12SquareCausalE" % ("int8" if a.variant == "fa_tc_int8_b" else "f16", a.d)
    res = {
        "tool": "causal_ab", "variant": a.variant, "B": a.B, "H": a.H, "N": a.N, "d": a.d,
        "rounds": a.rounds, "calls_per_round": a.calls,
        "main_kernel_ms": round(med[0][0], 5), "causal_main_kernel_ms": round(med[1][0], 5),
        "prepass_ms": round(med[0][1], 5), "causal_prepass_ms": round(med[1][1], 5),
        "call_ms": round(med[0][2], 5), "causal_call_ms": round(med[1][2], 5),
        "main_ratio": round(ratio, 4), "call_ratio": round(med[1][2] / med[0][2], 4),
        "main_ratio_per_round": [round(c[0] / n[0], 4) for n, c in zip(rows[0], rows[1])],
        "causal_waves": CAUSAL_WAVES, "R": round(R, 4), "bound_1p2R": round(1.2 * R, 4), "within_bound": ratio <= 1.2 * R,
        "clock_probe": bench.clock_probe(dev),
        "isa_sha16": {"main": ids.get("main", {}).get("isa_sha16"), "prepass": ids.get("prepass", {}).get("isa_sha16"),
                      "causal_main": isa_id.isa_sha16(_lib.LIB_PATH, ckern)},
        "device": torch.cuda.get_device_properties(dev).name,
    }
    print(json.dumps(res))


if __name__ == "__main__":
    main()
