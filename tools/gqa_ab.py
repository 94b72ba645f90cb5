#!/usr/bin/env python3
"""Grouped-query attention (qmha_kv_cache_create_gqa: h_kv K/V heads under H query heads) against the shipped
multi-head cache on K / V expanded to H heads, in one process, alternating.

    python tools/gqa_ab.py --variant fa_tc_int8_b --B 16 --H 16 --Hkv 4 --d 64 --len 4096 --row prefill decode

The reference is never the grouped path: it is the multi-head KVCache (the Rect kernels and the append pre-pass as
shipped before grouping existed) over K and V repeated G = H / h_kv times along the head axis, measured on the same
device in the same minute.  Both sides do the same step on a cache that already holds len - n rows: truncate (host
only) to len - n, append the n new rows, attend with the n queries (causal).  Rows:
  prefill   n = 1024: a prefill chunk behind len - 1024 cached rows
  decode    n = 32: one decode step at len
With qmha_profile on, both sides are warmed, then ROUNDS rounds alternate CALLS reference and CALLS candidate steps.
One JSON line per row: the per-round and median main-kernel, append and whole-step times of both sides (the library's
own event pairs), and
  main_ratio       grouped / multi-head main kernel
  ref_main_spread  the reference's (max - min) / median over its rounds 2.. (the first round after the warm-up is the
                   slow one); main_margin = 3 x that spread; main_not_slower = main_ratio <= 1 + main_margin, the one
                   criterion -- a miss is recorded with the per-round numbers, not tuned away
  append_ratio     grouped / multi-head append, reported against 1 / G (not gated: a decode append is launch-bound)
  cache_bytes      of both caches and their ratio (host arithmetic)
The grouped O is compared with the reference's bit for bit before anything is timed.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROWS = {"prefill": 1024, "decode": 32}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variant", default="fa_tc_int8_b", choices=["fa_tc_int8_b", "fa_tc_v1a"])
    ap.add_argument("--B", type=int, default=16)
    ap.add_argument("--H", type=int, default=16)
    ap.add_argument("--Hkv", type=int, default=4)
    ap.add_argument("--d", type=int, default=64)
    ap.add_argument("--len", type=int, default=4096, help="valid rows after the step's append (also the caches' cap)")
    ap.add_argument("--row", nargs="+", default=list(ROWS), choices=list(ROWS))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    if a.rounds < 5 or a.calls < 30:
        ap.error("at least 5 rounds of at least 30 calls")
    if a.Hkv < 1 or a.Hkv >= a.H or a.H % a.Hkv:
        ap.error("Hkv must be a proper divisor of H")
    if any(ROWS[r] >= a.len for r in a.row):
        ap.error("len must exceed the step's rows")

    import torch
    import bench
    from quantizedmha_amd import _lib, isa_id, torch_ext
    lib = _lib.load()
    dev = torch.device("cuda:0")
    G, dm, kvm, L = a.H // a.Hkv, a.H * a.d, a.Hkv * a.d, a.len
    gen = torch.Generator(device=dev).manual_seed(L + a.d + a.Hkv)
    K, V = (torch.rand((a.B, L, kvm), generator=gen, device=dev, dtype=torch.float32) for _ in range(2))

    def expanded(X):  # [B, n, h_kv d] -> [B, n, H d]
        b, n, _ = X.shape
        return X.view(b, n, a.Hkv, a.d).repeat_interleave(G, dim=2).reshape(b, n, dm).contiguous()

    vid = _lib.VARIANTS[a.variant]
    stream = torch.cuda.current_stream(dev).cuda_stream
    stem = "int8" if a.variant == "fa_tc_int8_b" else "f16"
    caches = {0: torch_ext.KVCache(a.B, L, dm, a.H, a.variant, device=dev),
              1: torch_ext.GroupedKVCache(a.B, L, dm, a.H, a.Hkv, a.variant, device=dev)}
    caches[0].append(expanded(K), expanded(V))
    caches[1].append(K, V)
    nbytes = {f: int(c.mem.numel()) for f, c in caches.items()}

    for row in a.row:
        n = ROWS[row]
        old = L - n
        Q = torch.rand((a.B, n, dm), generator=gen, device=dev, dtype=torch.float32)
        new = {1: (K[:, old:].contiguous(), V[:, old:].contiguous())}  # the step's new rows
        new[0] = tuple(expanded(x) for x in new[1])
        O = {0: torch.empty_like(Q), 1: torch.empty_like(Q)}

        def call(f):
            h = caches[f]._handle
            _lib.check(lib.qmha_kv_cache_truncate(h, old), "truncate")
            _lib.check(lib.qmha_kv_cache_append(h, new[f][0].data_ptr(), new[f][1].data_ptr(), n, stream), "append")
            _lib.check(lib.qmha_attend_cached(h, Q.data_ptr(), O[f].data_ptr(), n, _lib.QMHA_FLAG_CAUSAL, stream), "attend")

        def batch(f, k):
            """k steps: (main-kernel ms, append ms, whole-step ms), each per step."""
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(k):
                call(f)
            e1.record()
            torch.cuda.synchronize(dev)
            main_ms, pre_ms, recs = ctypes.c_double(), ctypes.c_double(), ctypes.c_longlong()
            _lib.check(lib.qmha_profile_collect(ctypes.byref(main_ms), ctypes.byref(recs), ctypes.byref(pre_ms)), "collect")
            assert recs.value == 2 * k, (recs.value, k)  # append and attend are a record each
            return main_ms.value / k, pre_ms.value / k, e0.elapsed_time(e1) / k

        for f in (0, 1):
            call(f)
        torch.cuda.synchronize(dev)
        bit_identical = bool(torch.equal(O[0], O[1]))
        lib.qmha_profile_collect(None, None, None)
        lib.qmha_profile_enable(1)
        try:
            for f in (0, 1):
                batch(f, a.warmup)
            rows = {0: [], 1: []}
            for _ in range(a.rounds):
                for f in (0, 1):
                    rows[f].append(batch(f, a.calls))
        finally:
            lib.qmha_profile_enable(0)
        med = {f: [statistics.median(r[i] for r in rows[f]) for i in range(3)] for f in rows}
        later = [r[0] for r in rows[0][1:]]
        spread = (max(later) - min(later)) / statistics.median(later)
        ratio = med[1][0] / med[0][0]
        res = {
            "tool": "gqa_ab", "row": row, "variant": a.variant, "B": a.B, "H": a.H, "h_kv": a.Hkv, "G": G, "d": a.d,
            "Nq": n, "len": L, "cap": L, "rounds": a.rounds, "calls_per_round": a.calls,
            "bit_identical_to_expanded_multi_head": bit_identical,
            "ref_main_kernel_ms": round(med[0][0], 5), "gqa_main_kernel_ms": round(med[1][0], 5),
            "ref_append_ms": round(med[0][1], 5), "gqa_append_ms": round(med[1][1], 5),
            "ref_step_ms": round(med[0][2], 5), "gqa_step_ms": round(med[1][2], 5),
            "main_ratio": round(ratio, 4), "ref_main_spread": round(spread, 4), "main_margin": round(3 * spread, 4),
            "main_not_slower": bool(ratio <= 1.0 + 3 * spread),
            "append_ratio": round(med[1][1] / med[0][1], 4), "append_ratio_expected": round(1.0 / G, 4),
            "step_ratio": round(med[1][2] / med[0][2], 4),
            "cache_bytes": {"ref": nbytes[0], "gqa": nbytes[1], "ratio": round(nbytes[1] / nbytes[0], 6)},
            "per_round": {"ref": [[round(x, 5) for x in r] for r in rows[0]],
                          "gqa": [[round(x, 5) for x in r] for r in rows[1]]},
            "clock_probe": bench.clock_probe(dev),
            "isa_sha16": {"ref_main": isa_id.isa_sha16(_lib.LIB_PATH, f"qmha_fa_{stem}_masked_kernelILi{a.d}ENS_4RectE"),
                          "gqa_main": isa_id.isa_sha16(_lib.LIB_PATH, f"qmha_fa_{stem}_masked_kernelILi{a.d}ENS_7GroupedE"),
                          "append": isa_id.isa_sha16(_lib.LIB_PATH, f"qmha_kv_append_{stem}_kernelILi{a.d}ENS_7HostRowE")},
            "device": torch.cuda.get_device_properties(dev).name,
        }
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
