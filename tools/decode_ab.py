#!/usr/bin/env python3
"""A decode step of an fp8 cache through the decode call (qmha_attend_cached_decode) against the step the
library offered before (qmha_attend_cached_tokens on the same cache), in one process, alternating; as context, the fp16
cache's attend_tokens_split at the same chunk_rows.

    python tools/decode_ab.py --B 16 --H 16 --d 64 --cap 4096 [--h-kv 4]

The shape of tools/split_ab.py: sequence b holds L[b] = 32 t[b] + 17 rows, t[b] spread evenly over 512 / 32 .. cap / 32 - 1
(B = 1: the longest); every step appends row L[b] - 1 again (append_tokens n = 1) and attends with one query row.  Before
anything is timed each candidate's O is held to the contract's restatement (tests/decode_ref.py) within the GPU tests' bound,
2 one-flip units + 2^-16 max|V|; a miss ends the run.  Then, with qmha_profile on, every side is warmed and ROUNDS rounds
alternate CALLS steps of each side; the figures are the library's own event pairs (one main pair around the partial and the
combine launch) and a device-event pair around each batch (the whole step).  Medians; the reference's round-to-round spread
(max - min) / median; a ratio counts as a gain only where every round lies below every round of the reference.  The HBM-time
floor is derived: the K/V bytes of the step's valid rows over --peak-gbs.  One JSON line.
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
    ap.add_argument("--B", type=int, default=16)
    ap.add_argument("--H", type=int, default=16)
    ap.add_argument("--h-kv", type=int, default=None, help="K/V heads of a grouped cache (default: H)")
    ap.add_argument("--d", type=int, default=64)
    ap.add_argument("--cap", type=int, default=4096)
    ap.add_argument("--chunks", type=int, nargs="+", default=[256, 512, 1024])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--peak-gbs", type=float, default=8000.0, help="HBM peak for the derived floor (MI355X data sheet: 8 TB/s)")
    a = ap.parse_args()
    if a.rounds < 5 or a.calls < 30:
        ap.error("at least 5 rounds of at least 30 calls")

    import numpy as np
    import torch
    import bench
    from quantizedmha_amd import _lib, isa_id, torch_ext
    from tests import decode_ref
    lib = _lib.load()
    dev = torch.device("cuda:0")
    hk = a.h_kv or a.H
    dm, kvm, r = a.H * a.d, hk * a.d, 17
    g = torch.Generator(device=dev).manual_seed(a.cap + a.d)
    K, V = (torch.rand((a.B, a.cap, kvm), generator=g, device=dev, dtype=torch.float32) for _ in range(2))
    q1 = torch.rand((a.B, 1, dm), generator=g, device=dev, dtype=torch.float32)
    stream = torch.cuda.current_stream(dev).cuda_stream
    CAUSAL = _lib.QMHA_FLAG_CAUSAL
    i32 = lambda xs: torch.tensor(xs, dtype=torch.int32, device=dev)  # noqa: E731

    t0, t1 = 512 // 32, a.cap // 32 - 1
    tiles = [t1] if a.B == 1 else [t0 + round(i * (t1 - t0) / (a.B - 1)) for i in range(a.B)]
    L = [32 * t + r for t in tiles]
    rows = lambda X, first, n: torch.stack([X[b, p:p + n] for b, p in enumerate(first)]).contiguous()  # noqa: E731
    scales = (1.0 / 256, 1.0 / 256, 1.0 / 256)  # U[0, 1) inputs over e4m3's range
    caches = {}
    for variant in ("fa_tc_fp8", "fa_tc_v1a"):
        c = torch_ext.GroupedKVCache(a.B, a.cap, dm, a.H, hk, variant, device=dev)
        if variant == "fa_tc_fp8":
            c.set_scales(*scales)
        c.append(K, V)
        c.enable_tokens()
        base = [32 * t for t in tiles]
        c.append_tokens(rows(K, base, r - 1), rows(V, base, r - 1), i32(base))  # the open group, from its first row on
        caches[variant] = c
    fp8, f16 = caches["fa_tc_fp8"], caches["fa_tc_v1a"]
    k1, v1 = rows(K, [x - 1 for x in L], 1), rows(V, [x - 1 for x in L], 1)
    pos1, lens1 = i32([x - 1 for x in L]), i32(L)
    outs = {s: torch.empty_like(q1) for s in ["ref"] + [f"decode{c}" for c in a.chunks] + [f"f16split{c}" for c in a.chunks]}
    dscr = {c: torch.zeros(lib.qmha_attend_decode_bytes(fp8._handle, 1, c), dtype=torch.uint8, device=dev) for c in a.chunks}
    sscr = {c: torch.zeros(lib.qmha_attend_split_bytes(f16._handle, 1, c), dtype=torch.uint8, device=dev) for c in a.chunks}

    def append(cache):
        _lib.check(lib.qmha_kv_cache_append_tokens(cache._handle, k1.data_ptr(), v1.data_ptr(), 1, pos1.data_ptr(), stream), "append_tokens")

    def ref_step():
        append(fp8)
        _lib.check(lib.qmha_attend_cached_tokens(fp8._handle, q1.data_ptr(), outs["ref"].data_ptr(), 1, lens1.data_ptr(), CAUSAL, stream),
                   "attend_tokens")

    def decode_step(c):
        def step():
            append(fp8)
            _lib.check(lib.qmha_attend_cached_decode(fp8._handle, q1.data_ptr(), outs[f"decode{c}"].data_ptr(), 1, lens1.data_ptr(), c,
                                                     dscr[c].data_ptr(), dscr[c].numel(), CAUSAL, stream), "attend_decode")
        return step

    def f16_step(c):
        def step():
            append(f16)
            _lib.check(lib.qmha_attend_cached_tokens_split(f16._handle, q1.data_ptr(), outs[f"f16split{c}"].data_ptr(), 1, lens1.data_ptr(), c,
                                                           sscr[c].data_ptr(), sscr[c].numel(), CAUSAL, stream), "attend_tokens_split")
        return step

    # ---- each candidate's O against the restatement, before anything is timed ----
    Qn, Kn, Vn = (x.cpu().numpy() for x in (q1, K, V))
    checks = {}
    for c in a.chunks:
        ref, _, Ltot, vmax = decode_ref.decode(Qn, Kn, Vn, L, a.H, hk, scales, c, a.cap)
        decode_step(c)()
        torch.cuda.synchronize(dev)
        got = outs[f"decode{c}"].cpu().numpy().astype(np.float64)
        bound = np.repeat(2.0 * 2.0 ** 4 * vmax[:, None, :] / Ltot, a.d, axis=-1) + 2.0 ** -16 * float(np.abs(Vn).max())
        checks[c] = {"finite": bool(np.isfinite(got).all()), "err_over_bound": round(float((np.abs(got - ref) / bound).max()), 4)}
    if not all(v["finite"] and v["err_over_bound"] <= 1.0 for v in checks.values()):
        print(json.dumps({"tool": "decode_ab", "checks": checks}), flush=True)
        sys.exit("decode_ab: a candidate's O is outside the restatement's bound")

    def batch(call, n):
        """n steps: (attend ms from the library's main pairs, append ms, whole-step ms) per step."""
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

    sides = {"ref": ref_step}  # the reference first
    sides.update({f"decode{c}": decode_step(c) for c in a.chunks})
    sides.update({f"f16split{c}": f16_step(c) for c in a.chunks})
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
    ref_main, ref_step_ms = [x[0] for x in per["ref"]], [x[2] for x in per["ref"]]
    spread = lambda xs, m: (max(xs) - min(xs)) / m  # noqa: E731
    kv_bytes = 2 * sum(-(-x // 32) * 32 for x in L) * hk * a.d  # e4m3 K and V^T of the tiles the step reads
    res = {"tool": "decode_ab", "B": a.B, "H": a.H, "h_kv": hk, "d": a.d, "cap": a.cap, "lens": L, "rounds": a.rounds,
           "calls_per_round": a.calls, "reference": "fp8 cache: append_tokens n=1 + attend_tokens Nq=1",
           "candidate": "fp8 cache: append_tokens n=1 + attend_decode Nq=1 (partial + combine)",
           "context": "fp16 cache: append_tokens n=1 + attend_tokens_split Nq=1", "checks": checks,
           "ref_attend_ms": round(med["ref"][0], 5), "ref_step_ms": round(med["ref"][2], 5), "append_ms": round(med["ref"][1], 5),
           "ref_attend_spread": round(spread(ref_main, med["ref"][0]), 4), "ref_step_spread": round(spread(ref_step_ms, med["ref"][2]), 4),
           "hbm_floor_ms_derived": round(kv_bytes / (a.peak_gbs * 1e9) * 1e3, 5), "kv_bytes": kv_bytes, "peak_gbs_assumed": a.peak_gbs,
           "sides": {}, "per_round": {s: [[round(x, 5) for x in row] for row in per[s]] for s in per},
           "clock_probe": bench.clock_probe(dev),
           "isa_sha16": {"fp8_ragged_main": isa_id.isa_sha16(_lib.LIB_PATH, f"qmha_fa_fp8_kernelINS_6RaggedELi{a.d}EEEv"),
                         "decode": isa_id.isa_sha16(_lib.LIB_PATH, f"qmha_fp8_decode_kernelINS_6RaggedELi{a.d}ELi{2 if a.H // hk > 16 else 1}EEEv"),
                         "combine": isa_id.isa_sha16(_lib.LIB_PATH, "qmha_split_combine_kernel")},
           "device": torch.cuda.get_device_properties(dev).name}
    lo_main, hi_main = min(ref_main), max(ref_main)
    lo_step, hi_step = min(ref_step_ms), max(ref_step_ms)
    for s in sides:
        if s == "ref":
            continue
        res["sides"][s] = {
            "attend_ms": round(med[s][0], 5), "step_ms": round(med[s][2], 5),
            "attend_ratio": round(med[s][0] / med["ref"][0], 4), "step_ratio": round(med[s][2] / med["ref"][2], 4),
            # every round of the side below (a gain) / above (a loss) every round of the reference
            "attend_verdict": "gain" if max(x[0] for x in per[s]) < lo_main else "loss" if min(x[0] for x in per[s]) > hi_main else "inside the spread",
            "step_verdict": "gain" if max(x[2] for x in per[s]) < lo_step else "loss" if min(x[2] for x in per[s]) > hi_step else "inside the spread"}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
