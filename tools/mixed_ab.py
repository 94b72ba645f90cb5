#!/usr/bin/env python3
"""A continuous-batching step of an fp8 cache through the mixed-step attend (qmha_attend_cached_mixed) against the
calls that served it before, in one process, alternating.

    python tools/mixed_ab.py --B 16 --H 16 --d 64 --cap 4096 [--h-kv 4]

Sequence b holds L_b = 32 t_b + 17 rows, t_b spread over 512 ... cap.  The step: the first and the last sequence bring a
prefill chunk of --nq rows (default 512), every other one decode row.  Reference, per window (default 128, 1024, cap) with a
per-head ramp of sinks: attend_prefill_window at Nq = nq plus attend_decode_window at Nq = 1, each with the other kind's
sequences switched off through lens = 0 -- two calls, three launches where the decode call combines.  Control: an all-decode
step against attend_decode_window alone.  Before anything is timed the mixed call's O is held bit for bit to the reference
route's rows; a miss ends the run.  Then, with qmha_profile on, every side is warmed and ROUNDS rounds alternate CALLS steps of
each side; the figures are the library's own event pairs, summed per step.  Medians; the reference's round-to-round spread
(max - min) / median; a ratio counts as a gain only where every round lies below every round of the reference.  One JSON line.
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
    ap.add_argument("--nq", type=int, default=512)
    ap.add_argument("--chunk-rows", type=int, default=512)
    ap.add_argument("--windows", type=int, nargs="+", default=None, help="default: 128 1024 cap")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    if a.rounds < 5 or a.calls < 30 or a.B < 3:
        ap.error("at least 5 rounds of at least 30 calls, at least 3 sequences")

    import torch
    import bench
    from quantizedmha_amd import _lib, isa_id, torch_ext
    lib = _lib.load()
    dev = torch.device("cuda:0")
    hk, windows = a.h_kv or a.H, a.windows or [128, 1024, a.cap]
    dm, kvm = a.H * a.d, hk * a.d
    t_lo, t_hi = -(-max(512, a.nq) // 32), (a.cap - 17) // 32
    L = [32 * (t_lo + (t_hi - t_lo) * b // (a.B - 1)) + 17 for b in range(a.B)]
    g = torch.Generator(device=dev).manual_seed(a.cap + a.d)
    K, V = (torch.rand((a.B, a.cap, kvm), generator=g, device=dev, dtype=torch.float32) for _ in range(2))
    sinks = torch.linspace(-2.0, 3.0, a.H, device=dev, dtype=torch.float32)
    stream = torch.cuda.current_stream(dev).cuda_stream
    CAUSAL = _lib.QMHA_FLAG_CAUSAL
    fp8 = torch_ext.GroupedKVCache(a.B, a.cap, dm, a.H, hk, "fa_tc_fp8", device=dev)
    fp8.set_scales(1.0 / 256, 1.0 / 256, 1.0 / 256)  # U[0, 1) inputs over e4m3's range
    fp8.append(K, V)
    i32 = lambda xs: torch.tensor(xs, dtype=torch.int32, device=dev)  # noqa: E731
    mscr = torch.zeros(lib.qmha_attend_mixed_bytes(fp8._handle, max(windows), a.chunk_rows), dtype=torch.uint8, device=dev)
    dscr = torch.zeros(lib.qmha_attend_decode_window_bytes(fp8._handle, 1, max(windows), a.chunk_rows), dtype=torch.uint8, device=dev)

    def step(counts):
        """The operands of one mix: packed Q / O and cu for the mixed call, batched Q / O and lens for the reference route."""
        cu = [0]
        for n in counts:
            cu.append(cu[-1] + n)
        s = {"counts": counts, "cu": i32(cu), "lens": i32(L), "Q": torch.rand((cu[-1], dm), generator=g, device=dev, dtype=torch.float32)}
        s["O"] = torch.zeros_like(s["Q"])
        for kind, n in (("pre", a.nq), ("dec", 1)):
            idx = [b for b in range(a.B) if counts[b] == n]
            if idx:
                Qk = torch.zeros((a.B, n, dm), device=dev, dtype=torch.float32)
                for b in idx:
                    Qk[b] = s["Q"][cu[b]:cu[b + 1]]
                s[kind] = (Qk, torch.zeros_like(Qk), i32([L[b] if b in idx else 0 for b in range(a.B)]), idx)
        return s

    def mixed_call(s, w):
        def call():
            _lib.check(lib.qmha_attend_cached_mixed(fp8._handle, s["Q"].data_ptr(), s["O"].data_ptr(), s["Q"].shape[0], s["cu"].data_ptr(),
                                                    s["lens"].data_ptr(), w, sinks.data_ptr(), a.chunk_rows, mscr.data_ptr(), mscr.numel(), CAUSAL,
                                                    stream), "attend_mixed")
        return call, 1

    def ref_call(s, w):
        def call():
            if "pre" in s:
                Qk, Ok, lens, _ = s["pre"]
                _lib.check(lib.qmha_attend_cached_prefill_window(fp8._handle, Qk.data_ptr(), Ok.data_ptr(), a.nq, lens.data_ptr(), w, sinks.data_ptr(),
                                                                 CAUSAL, stream), "attend_prefill_window")
            Qk, Ok, lens, _ = s["dec"]
            _lib.check(lib.qmha_attend_cached_decode_window(fp8._handle, Qk.data_ptr(), Ok.data_ptr(), 1, lens.data_ptr(), w, sinks.data_ptr(),
                                                            a.chunk_rows, dscr.data_ptr(), dscr.numel(), CAUSAL, stream), "attend_decode_window")
        return call, 2 if "pre" in s else 1

    steps = {"mix": step([a.nq if b in (0, a.B - 1) else 1 for b in range(a.B)]), "decode": step([1] * a.B)}
    sides, checks = {}, {}
    for sname, s in steps.items():
        for w in windows:
            sides[f"{sname}_ref_w{w}"], sides[f"{sname}_mixed_w{w}"] = ref_call(s, w), mixed_call(s, w)
            # ---- bit for bit against the reference route, before anything is timed ----
            sides[f"{sname}_ref_w{w}"][0](), sides[f"{sname}_mixed_w{w}"][0]()
            torch.cuda.synchronize(dev)
            cu = s["cu"].tolist()
            same = all(torch.equal(s["O"][cu[b]:cu[b + 1]], s[kind][1][b]) for kind in ("pre", "dec") if kind in s for b in s[kind][3])
            checks[f"{sname}_w{w}"] = {"finite": bool(torch.isfinite(s["O"]).all()), "bits_equal": bool(same)}
    if not all(v["finite"] and v["bits_equal"] for v in checks.values()):
        print(json.dumps({"tool": "mixed_ab", "checks": checks}), flush=True)
        sys.exit("mixed_ab: the mixed call's O is not the reference route's")

    def batch(side, n):
        """n steps: ms per step from the library's main pairs."""
        call, pairs = side
        for _ in range(n):
            call()
        torch.cuda.synchronize(dev)
        main_ms, pre_ms, k = ctypes.c_double(), ctypes.c_double(), ctypes.c_longlong()
        _lib.check(lib.qmha_profile_collect(ctypes.byref(main_ms), ctypes.byref(k), ctypes.byref(pre_ms)), "collect")
        assert k.value == n * pairs, (k.value, n, pairs)
        return main_ms.value / n

    lib.qmha_profile_collect(None, None, None)
    lib.qmha_profile_enable(1)
    try:
        for side in sides.values():
            batch(side, a.warmup)
        per = {s: [] for s in sides}
        for _ in range(a.rounds):
            for s, side in sides.items():
                per[s].append(batch(side, a.calls))
    finally:
        lib.qmha_profile_enable(0)
    med = {s: statistics.median(per[s]) for s in per}
    res = {"tool": "mixed_ab", "B": a.B, "H": a.H, "h_kv": hk, "d": a.d, "cap": a.cap, "nq": a.nq, "chunk_rows": a.chunk_rows, "lens": L,
           "rounds": a.rounds, "calls_per_round": a.calls, "reference": "attend_prefill_window Nq=nq + attend_decode_window Nq=1, the other kind switched off",
           "candidate": "attend_mixed", "timing": "sum of the library's main event pairs per step; gaps between a step's calls are not in it",
           "checks": checks, "results": {}, "per_round": {s: [round(x, 5) for x in per[s]] for s in per}, "clock_probe": bench.clock_probe(dev),
           "isa_sha16": {"mixed": isa_id.isa_sha16(_lib.LIB_PATH, f"qmha_fp8_mixed_kernelINS_6RaggedELi{a.d}EEEv"),
                         "band": isa_id.isa_sha16(_lib.LIB_PATH, f"qmha_fp8_band_kernelINS_6RaggedELi{a.d}EEEv")},
           "device": torch.cuda.get_device_properties(dev).name}
    for sname in steps:
        for w in windows:
            r, m = per[f"{sname}_ref_w{w}"], per[f"{sname}_mixed_w{w}"]
            mr = statistics.median(r)
            # every round of the mixed call below (a gain) / above (a loss) every round of the reference
            res["results"][f"{sname}_w{w}"] = {"ref_ms": round(mr, 5), "ref_spread": round((max(r) - min(r)) / mr, 4), "mixed_ms": round(statistics.median(m), 5),
                                               "ratio": round(statistics.median(m) / mr, 4),
                                               "verdict": "gain" if max(m) < min(r) else "loss" if min(m) > max(r) else "inside the spread"}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
