#!/usr/bin/env python3
"""Rectangular attention (qmha_solve_rect, Nq != Nk) against the shipped square kernels at N = Nk, in one
process, alternating.

    python tools/rect_ab.py --variant fa_tc_int8_b --B 16 --H 16 --Nq 1024 --Nk 4096 --d 64 --causal

The reference time is a kernel the parent commit ships, measured on the same device in the same minute: with
--causal the square causal kernel (qmha_solve_opts(QMHA_FLAG_CAUSAL)) at N = Nk, without it the non-causal
main kernel at N = Nk.  With qmha_profile on, both sides are warmed, then ROUNDS rounds alternate CALLS square
and CALLS rectangular calls; the medians over the rounds of the per-call main-kernel time (the library's own
event pairs), pre-pass time and whole-call time are printed as one JSON line with their ratios.
The expected ratio is the workgroup-level tile ratio R: a workgroup's KV loop runs to its last wave's last
tile, so with WAVES query groups per workgroup, Gq = Nq / 32, Gk = Nk / 32 and nqb(G) = ceil(G / WAVES)
    causal       rect: sum_qb min(Gk, Gk - Gq + WAVES (qb + 1)) over nqb(Gq);  square: sum_qb min(Gk, WAVES (qb + 1)) over nqb(Gk)
    non-causal   rect: Gk nqb(Gq);                                             square: Gk nqb(Gk)
and R = rect / square.  DESIGN.md 11 holds the measured main-kernel ratio to 1.2 R.
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
    RECT_WAVES = int(re.search(r"constexpr int kWaves = (\d+)", _f.read()).group(1))


def tiles(Nq, Nk, causal, waves=RECT_WAVES):
    """Workgroup-level tile count of one (b, h): every q-block's KV loop length, summed."""
    Gq, Gk = Nq // 32, Nk // 32
    nqb = (Gq + waves - 1) // waves
    if not causal:
        return nqb * Gk
    return sum(min(Gk, Gk - Gq + waves * (qb + 1)) for qb in range(nqb))


def tile_ratio(Nq, Nk, causal):
    return tiles(Nq, Nk, causal) / tiles(Nk, Nk, causal)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variant", default="fa_tc_int8_b", choices=["fa_tc_int8_b", "fa_tc_v1a"])
    ap.add_argument("--B", type=int, default=16)
    ap.add_argument("--H", type=int, default=16)
    ap.add_argument("--Nq", type=int, default=1024)
    ap.add_argument("--Nk", type=int, default=4096)
    ap.add_argument("--d", type=int, default=64)
    ap.add_argument("--causal", action="store_true")
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
    g = torch.Generator(device=dev).manual_seed(a.Nq + a.Nk + a.d)
    K, V = (torch.rand((a.B, a.Nk, dm), generator=g, device=dev, dtype=torch.float32) for _ in range(2))
    Qs = torch.rand((a.B, a.Nk, dm), generator=g, device=dev, dtype=torch.float32)  # the square call's queries
    Qr = Qs[:, a.Nk - a.Nq:].contiguous() if a.Nq <= a.Nk else torch.rand((a.B, a.Nq, dm), generator=g, device=dev)
    Os, Or = torch.empty_like(Qs), torch.empty_like(Qr)
    vid = _lib.VARIANTS[a.variant]
    flags = _lib.QMHA_FLAG_CAUSAL if a.causal else 0
    stream = torch.cuda.current_stream(dev).cuda_stream

    def call(rect):
        if rect:
            st = lib.qmha_solve_rect(Qr.data_ptr(), K.data_ptr(), V.data_ptr(), Or.data_ptr(), a.B, a.Nq, a.Nk, dm, a.H,
                                     vid, flags, None, 0, stream)
        else:
            st = lib.qmha_solve_opts(Qs.data_ptr(), K.data_ptr(), V.data_ptr(), Os.data_ptr(), a.B, a.Nk, dm, a.H, vid,
                                     flags, None, 0, stream)
        _lib.check(st, "rect_ab")

    def batch(rect, n):
        """n calls: (main-kernel ms per call, pre-pass ms per call, whole-call ms per call)."""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            call(rect)
        e1.record()
        torch.cuda.synchronize(dev)
        main_ms, pre_ms, k = ctypes.c_double(), ctypes.c_double(), ctypes.c_longlong()
        _lib.check(lib.qmha_profile_collect(ctypes.byref(main_ms), ctypes.byref(k), ctypes.byref(pre_ms)), "collect")
        assert k.value == n, (k.value, n)
        return main_ms.value / n, pre_ms.value / n, e0.elapsed_time(e1) / n

    lib.qmha_profile_collect(None, None, None)
    lib.qmha_profile_enable(1)
    try:
        for rect in (0, 1):
            batch(rect, a.warmup)
        rows = {0: [], 1: []}
        for _ in range(a.rounds):
            for rect in (0, 1):
                rows[rect].append(batch(rect, a.calls))
    finally:
        lib.qmha_profile_enable(0)
    med = {f: [statistics.median(r[i] for r in rows[f]) for i in range(3)] for f in rows}
    R = tile_ratio(a.Nq, a.Nk, a.causal)
    ratio = med[1][0] / med[0][0]
    ids = bench.isa_ids(a.variant, a.d)
    stem = "int8" if a.variant == "fa_tc_int8_b" else "f16"
    ref_main = isa_id.isa_sha16(_lib.LIB_PATH, f"qmha_fa_{stem}_masked_kernelILi{a.d}ENS_12SquareCausalE") if a.causal else \
        ids.get("main", {}).get("isa_sha16")
    res = {
        "tool": "rect_ab", "variant": a.variant, "B": a.B, "H": a.H, "Nq": a.Nq, "Nk": a.Nk, "d": a.d, "causal": a.causal,
        "rounds": a.rounds, "calls_per_round": a.calls,
        "square_main_kernel_ms": round(med[0][0], 5), "rect_main_kernel_ms": round(med[1][0], 5),
        "square_prepass_ms": round(med[0][1], 5), "rect_prepass_ms": round(med[1][1], 5),
        "square_call_ms": round(med[0][2], 5), "rect_call_ms": round(med[1][2], 5),
        "main_ratio": round(ratio, 4), "call_ratio": round(med[1][2] / med[0][2], 4),
        "rect_prepass_share_of_call": round(med[1][1] / med[1][2], 4),
        "main_ratio_per_round": [round(r[0] / s[0], 4) for s, r in zip(rows[0], rows[1])],
        "rect_waves": RECT_WAVES, "R": round(R, 4), "bound_1p2R": round(1.2 * R, 4), "within_bound": ratio <= 1.2 * R,
        "clock_probe": bench.clock_probe(dev),
        "isa_sha16": {"square_main": ref_main, "prepass": ids.get("prepass", {}).get("isa_sha16"),
                      "rect_main": isa_id.isa_sha16(_lib.LIB_PATH, f"qmha_fa_{stem}_masked_kernelILi{a.d}ENS_4RectE")},
        "device": torch.cuda.get_device_properties(dev).name,
    }
    print(json.dumps(res))


if __name__ == "__main__":
    main()
