#!/usr/bin/env python3
"""The persistent K/V cache (qmha_kv_cache_append + qmha_attend_cached) against qmha_solve_rect, in one process,
alternating.

    python tools/kvcache_ab.py --variant fa_tc_int8_b --B 16 --H 16 --Nq 1024 --Nk 4096 --d 64 --cap 4096 8192

The reference is what the library ships without a cache, measured on the same device in the same minute: the last
chunk of a chunked prefill as qmha_solve_rect(Nq, Nk, QMHA_FLAG_CAUSAL), whose pre-pass runs over all Nk rows.  The
candidate is the same chunk through a cache of `cap` rows that already holds the first Nk - Nq: truncate (host only)
to Nk - Nq, append the Nq new rows, attend with the Nq queries.  With qmha_profile on, both sides are warmed, then
ROUNDS rounds alternate CALLS reference and CALLS candidate calls.  One JSON line per cap: the per-round and median
main-kernel, pre-pass and whole-call times of both sides (the library's own event pairs), and
  main_ratio            cached / rect main kernel: the same machine code over the same tiles, expected 1 within the
                        reference's own round-to-round spread (ref_main_spread = (max - min) / median of its rounds)
  prepass_ratio         append / rect pre-pass, against the HBM-bound expectation Nq / Nk
  call_ratio            whole call
The candidate's O is compared with the reference's bit for bit before anything is timed.
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
    ap.add_argument("--Nq", type=int, default=1024)
    ap.add_argument("--Nk", type=int, default=4096)
    ap.add_argument("--d", type=int, default=64)
    ap.add_argument("--cap", type=int, nargs="+", default=[4096, 8192])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    if a.rounds < 5 or a.calls < 30:
        ap.error("at least 5 rounds of at least 30 calls")
    if not 0 < a.Nq < a.Nk or any(c < a.Nk for c in a.cap):
        ap.error("0 < Nq < Nk <= cap")

    import torch
    import bench
    from quantizedmha_amd import _lib, isa_id, torch_ext
    lib = _lib.load()
    dev = torch.device("cuda:0")
    dm = a.H * a.d
    g = torch.Generator(device=dev).manual_seed(a.Nq + a.Nk + a.d)
    K, V = (torch.rand((a.B, a.Nk, dm), generator=g, device=dev, dtype=torch.float32) for _ in range(2))
    Q = torch.rand((a.B, a.Nq, dm), generator=g, device=dev, dtype=torch.float32)
    old = a.Nk - a.Nq
    Kn, Vn = K[:, old:].contiguous(), V[:, old:].contiguous()  # the chunk's new rows
    Or, Oc = torch.empty_like(Q), torch.empty_like(Q)
    vid = _lib.VARIANTS[a.variant]
    stream = torch.cuda.current_stream(dev).cuda_stream
    stem = "int8" if a.variant == "fa_tc_int8_b" else "f16"

    for cap in a.cap:
        cache = torch_ext.KVCache(a.B, cap, dm, a.H, a.variant, device=dev)
        cache.append(K[:, :old].contiguous(), V[:, :old].contiguous())
        handle = cache._handle

        def call(cached):
            if cached:
                _lib.check(lib.qmha_kv_cache_truncate(handle, old), "truncate")
                _lib.check(lib.qmha_kv_cache_append(handle, Kn.data_ptr(), Vn.data_ptr(), a.Nq, stream), "append")
                st = lib.qmha_attend_cached(handle, Q.data_ptr(), Oc.data_ptr(), a.Nq, _lib.QMHA_FLAG_CAUSAL, stream)
            else:
                st = lib.qmha_solve_rect(Q.data_ptr(), K.data_ptr(), V.data_ptr(), Or.data_ptr(), a.B, a.Nq, a.Nk, dm, a.H,
                                         vid, _lib.QMHA_FLAG_CAUSAL, None, 0, stream)
            _lib.check(st, "kvcache_ab")

        def batch(cached, n):
            """n calls: (main-kernel ms per call, pre-pass ms per call, whole-call ms per call)."""
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(n):
                call(cached)
            e1.record()
            torch.cuda.synchronize(dev)
            main_ms, pre_ms, k = ctypes.c_double(), ctypes.c_double(), ctypes.c_longlong()
            _lib.check(lib.qmha_profile_collect(ctypes.byref(main_ms), ctypes.byref(k), ctypes.byref(pre_ms)), "collect")
            assert k.value == (2 * n if cached else n), (k.value, n)  # append and attend are a record each
            return main_ms.value / n, pre_ms.value / n, e0.elapsed_time(e1) / n

        for cached in (0, 1):
            call(cached)
        torch.cuda.synchronize(dev)
        bit_identical = bool(torch.equal(Or, Oc))
        lib.qmha_profile_collect(None, None, None)
        lib.qmha_profile_enable(1)
        try:
            for cached in (0, 1):
                batch(cached, a.warmup)
            rows = {0: [], 1: []}
            for _ in range(a.rounds):
                for cached in (0, 1):
                    rows[cached].append(batch(cached, a.calls))
        finally:
            lib.qmha_profile_enable(0)
        med = {f: [statistics.median(r[i] for r in rows[f]) for i in range(3)] for f in rows}
        ref_main = [r[0] for r in rows[0]]
        res = {
            "tool": "kvcache_ab", "variant": a.variant, "B": a.B, "H": a.H, "Nq": a.Nq, "Nk": a.Nk, "d": a.d, "cap": cap,
            "rounds": a.rounds, "calls_per_round": a.calls, "bit_identical_to_rect": bit_identical,
            "rect_main_kernel_ms": round(med[0][0], 5), "cached_main_kernel_ms": round(med[1][0], 5),
            "rect_prepass_ms": round(med[0][1], 5), "append_prepass_ms": round(med[1][1], 5),
            "rect_call_ms": round(med[0][2], 5), "cached_call_ms": round(med[1][2], 5),
            "main_ratio": round(med[1][0] / med[0][0], 4),
            "ref_main_spread": round((max(ref_main) - min(ref_main)) / med[0][0], 4),
            "prepass_ratio": round(med[1][1] / med[0][1], 4), "prepass_ratio_expected": round(a.Nq / a.Nk, 4),
            "call_ratio": round(med[1][2] / med[0][2], 4),
            "per_round": {"rect": [[round(x, 5) for x in r] for r in rows[0]],
                          "cached": [[round(x, 5) for x in r] for r in rows[1]]},
            "clock_probe": bench.clock_probe(dev),
            "isa_sha16": {"main": isa_id.isa_sha16(_lib.LIB_PATH, f"qmha_fa_{stem}_masked_kernelILi{a.d}ENS_4RectE"),
                          "prepass": bench.isa_ids(a.variant, a.d).get("prepass", {}).get("isa_sha16"),
                          "append": isa_id.isa_sha16(_lib.LIB_PATH, f"qmha_kv_append_{stem}_kernelILi{a.d}ENS_7HostRowE")},
            "device": torch.cuda.get_device_properties(dev).name,
        }
        print(json.dumps(res), flush=True)
        del cache


if __name__ == "__main__":
    main()
