#!/usr/bin/env python3
"""A decode step of an fp8 cache through the windowed decode call (qmha_attend_cached_decode_window) against the
unwindowed decode call (qmha_attend_cached_decode) on the same cache, in one process, alternating.

    python tools/decode_window_ab.py --B 16 --H 16 --d 64 --cap 4096 [--h-kv 4]

The shape of tools/decode_ab.py: sequence b holds L[b] = 32 t[b] + 17 rows, t[b] spread evenly over 512 / 32 .. cap / 32 - 1
(B = 1: the longest); every step appends row L[b] - 1 again (append_tokens n = 1) and attends with one query row.  Candidates
are (window, chunk_rows) pairs: window 128 in the one-launch form (chunk_rows 256) and in the combine form (64), 1024 at 256
and 512, and a window of cap at the reference's chunk_rows, where the call does the reference's work.  Before anything is
timed each candidate's O is held to the contract's restatement (tests/decode_window_ref.py, with a per-head ramp of sinks)
within the GPU tests' bound, 2 one-flip units + 2^-16 max|V|; a miss ends the run.  Then, with qmha_profile on, every side is
warmed and ROUNDS rounds alternate CALLS steps of each side; the figures are the library's own event pairs (one main pair
around a call's launches) and a device-event pair around each batch (the whole step).  Medians; the reference's
round-to-round spread (max - min) / median; a ratio counts as a gain only where every round lies below every round of the
reference.  tile_ratio is derived: the tiles a candidate sweeps over the tiles of the full sweep.  One JSON line.
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
    ap.add_argument("--ref-chunk", type=int, default=1024, help="chunk_rows of the reference and of the window-of-cap candidate")
    ap.add_argument("--pairs", type=int, nargs="+", default=[128, 256, 128, 64, 1024, 256, 1024, 512], help="window chunk_rows ...")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    if a.rounds < 5 or a.calls < 30 or len(a.pairs) % 2:
        ap.error("at least 5 rounds of at least 30 calls; --pairs takes window chunk_rows pairs")

    import numpy as np
    import torch
    import bench
    from quantizedmha_amd import _lib, isa_id, torch_ext
    from tests import decode_window_ref as ref
    lib = _lib.load()
    dev = torch.device("cuda:0")
    hk = a.h_kv or a.H
    dm, kvm, r = a.H * a.d, hk * a.d, 17
    g = torch.Generator(device=dev).manual_seed(a.cap + a.d)
    K, V = (torch.rand((a.B, a.cap, kvm), generator=g, device=dev, dtype=torch.float32) for _ in range(2))
    q1 = torch.rand((a.B, 1, dm), generator=g, device=dev, dtype=torch.float32)
    sinks = torch.linspace(-2.0, 3.0, a.H, device=dev, dtype=torch.float32)
    stream = torch.cuda.current_stream(dev).cuda_stream
    CAUSAL = _lib.QMHA_FLAG_CAUSAL
    i32 = lambda xs: torch.tensor(xs, dtype=torch.int32, device=dev)  # noqa: E731

    t0, t1 = 512 // 32, a.cap // 32 - 1
    tiles = [t1] if a.B == 1 else [t0 + round(i * (t1 - t0) / (a.B - 1)) for i in range(a.B)]
    L = [32 * t + r for t in tiles]
    rows = lambda X, first, n: torch.stack([X[b, p:p + n] for b, p in enumerate(first)]).contiguous()  # noqa: E731
    scales = (1.0 / 256, 1.0 / 256, 1.0 / 256)  # U[0, 1) inputs over e4m3's range
    fp8 = torch_ext.GroupedKVCache(a.B, a.cap, dm, a.H, hk, "fa_tc_fp8", device=dev)
    fp8.set_scales(*scales)
    fp8.append(K, V)
    fp8.enable_tokens()
    base = [32 * t for t in tiles]
    fp8.append_tokens(rows(K, base, r - 1), rows(V, base, r - 1), i32(base))  # the open group, from its first row on
    k1, v1 = rows(K, [x - 1 for x in L], 1), rows(V, [x - 1 for x in L], 1)
    pos1, lens1 = i32([x - 1 for x in L]), i32(L)
    pairs = list(zip(a.pairs[::2], a.pairs[1::2])) + [(a.cap, a.ref_chunk)]
    name = lambda w, c: f"window{w}_chunk{c}"  # noqa: E731
    outs = {s: torch.empty_like(q1) for s in ["ref"] + [name(*p) for p in pairs]}
    rscr = torch.zeros(lib.qmha_attend_decode_bytes(fp8._handle, 1, a.ref_chunk), dtype=torch.uint8, device=dev)
    wscr = {p: torch.zeros(lib.qmha_attend_decode_window_bytes(fp8._handle, 1, *p), dtype=torch.uint8, device=dev) for p in pairs}

    def append():
        _lib.check(lib.qmha_kv_cache_append_tokens(fp8._handle, k1.data_ptr(), v1.data_ptr(), 1, pos1.data_ptr(), stream), "append_tokens")

    def ref_step():
        append()
        _lib.check(lib.qmha_attend_cached_decode(fp8._handle, q1.data_ptr(), outs["ref"].data_ptr(), 1, lens1.data_ptr(), a.ref_chunk,
                                                 rscr.data_ptr(), rscr.numel(), CAUSAL, stream), "attend_decode")

    def window_step(w, c):
        def step():
            append()
            _lib.check(lib.qmha_attend_cached_decode_window(fp8._handle, q1.data_ptr(), outs[name(w, c)].data_ptr(), 1, lens1.data_ptr(), w,
                                                            sinks.data_ptr(), c, wscr[w, c].data_ptr(), wscr[w, c].numel(), CAUSAL, stream),
                       "attend_decode_window")
        return step

    # ---- each candidate's O against the restatement, before anything is timed ----
    Qn, Kn, Vn, Sn = (x.cpu().numpy() for x in (q1, K, V, sinks))
    checks, forms, tile_ratio = {}, {}, {}
    for w, c in pairs:
        want, _, Ltot, vmax = ref.decode_window(Qn, Kn, Vn, L, a.H, hk, scales, c, a.cap, w, Sn)
        window_step(w, c)()
        torch.cuda.synchronize(dev)
        got = outs[name(w, c)].cpu().numpy().astype(np.float64)
        bound = np.repeat(2.0 * 2.0 ** 4 * vmax[:, None, :] / Ltot, a.d, axis=-1) + 2.0 ** -16 * float(np.abs(Vn).max())
        checks[name(w, c)] = {"finite": bool(np.isfinite(got).all()), "err_over_bound": round(float((np.abs(got - want) / bound).max()), 4)}
        forms[name(w, c)] = "one launch" if ref.chunks(a.cap, 1, w, c) == 1 else f"combine over {ref.chunks(a.cap, 1, w, c)} chunks"
        tile_ratio[name(w, c)] = round(sum((x - 1) // 32 - ref.first_tile(x, 1, w) + 1 for x in L) / sum((x - 1) // 32 + 1 for x in L), 4)
    if not all(v["finite"] and v["err_over_bound"] <= 1.0 for v in checks.values()):
        print(json.dumps({"tool": "decode_window_ab", "checks": checks}), flush=True)
        sys.exit("decode_window_ab: a candidate's O is outside the restatement's bound")

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
    sides.update({name(*p): window_step(*p) for p in pairs})
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
    qb = 2 if a.H // hk > 16 else 1
    res = {"tool": "decode_window_ab", "B": a.B, "H": a.H, "h_kv": hk, "d": a.d, "cap": a.cap, "lens": L, "rounds": a.rounds,
           "calls_per_round": a.calls, "reference": f"append_tokens n=1 + attend_decode Nq=1 at chunk_rows {a.ref_chunk}",
           "candidate": "append_tokens n=1 + attend_decode_window Nq=1 with sinks", "checks": checks, "forms": forms, "tile_ratio_derived": tile_ratio,
           "ref_attend_ms": round(med["ref"][0], 5), "ref_step_ms": round(med["ref"][2], 5), "append_ms": round(med["ref"][1], 5),
           "ref_attend_spread": round(spread(ref_main, med["ref"][0]), 4), "ref_step_spread": round(spread(ref_step_ms, med["ref"][2]), 4),
           "sides": {}, "per_round": {s: [[round(x, 5) for x in row] for row in per[s]] for s in per},
           "clock_probe": bench.clock_probe(dev),
           "isa_sha16": {"decode": isa_id.isa_sha16(_lib.LIB_PATH, f"qmha_fp8_decode_kernelINS_6RaggedELi{a.d}ELi{qb}EEEv"),
                         "window_direct": isa_id.isa_sha16(_lib.LIB_PATH, f"qmha_fp8_decode_window_kernelINS_6RaggedELi{a.d}ELi{qb}ELb1EEEv"),
                         "window_partial": isa_id.isa_sha16(_lib.LIB_PATH, f"qmha_fp8_decode_window_kernelINS_6RaggedELi{a.d}ELi{qb}ELb0EEEv"),
                         "window_combine": isa_id.isa_sha16(_lib.LIB_PATH, "qmha_fp8_decode_window_combine_kernel")},
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
