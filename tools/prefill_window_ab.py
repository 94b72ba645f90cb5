#!/usr/bin/env python3
"""A prefill chunk of an fp8 cache through the windowed prefill call (qmha_attend_cached_prefill_window) against
attend_tokens (qmha_attend_cached_tokens) on the same cache, in one process, alternating.

    python tools/prefill_window_ab.py --B 16 --H 16 --d 64 --cap 4096 [--h-kv 4]

Every sequence holds L = cap rows and attends with one chunk of Nq query rows (default 1024).  Candidates are windows (default
128, 1024 and cap, where the call does the reference's work) with a per-head ramp of sinks.  Before anything is timed each
candidate's O -- sequence 0, the first and the last head -- is held to the contract's restatement (tests/prefill_window_ref.py)
within the GPU tests' bound, 2 one-flip units + 2^-16 max|V|; a miss ends the run.  Then, with qmha_profile on, every side is
warmed and ROUNDS rounds alternate CALLS calls of each side; the figures are the library's own event pairs (one main pair per
call).  Medians; the reference's round-to-round spread (max - min) / median; a ratio counts as a gain only where every round
lies below every round of the reference.  tile_ratio is derived: the tiles a candidate's query groups sweep over the tiles of
the full causal sweep.  One JSON line.
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
    ap.add_argument("--nq", type=int, default=1024)
    ap.add_argument("--windows", type=int, nargs="+", default=None, help="default: 128 1024 cap")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    if a.rounds < 5 or a.calls < 30:
        ap.error("at least 5 rounds of at least 30 calls")

    import numpy as np
    import torch
    import bench
    from quantizedmha_amd import _lib, isa_id, torch_ext
    from tests import prefill_window_ref as ref
    lib = _lib.load()
    dev = torch.device("cuda:0")
    hk, L, windows = a.h_kv or a.H, a.cap, a.windows or [128, 1024, a.cap]
    G, dm, kvm = a.H // hk, a.H * a.d, hk * a.d
    g = torch.Generator(device=dev).manual_seed(a.cap + a.d)
    K, V = (torch.rand((a.B, a.cap, kvm), generator=g, device=dev, dtype=torch.float32) for _ in range(2))
    Q = torch.rand((a.B, a.nq, dm), generator=g, device=dev, dtype=torch.float32)
    sinks = torch.linspace(-2.0, 3.0, a.H, device=dev, dtype=torch.float32)
    lens = torch.full((a.B,), L, dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    CAUSAL = _lib.QMHA_FLAG_CAUSAL
    scales = (1.0 / 256, 1.0 / 256, 1.0 / 256)  # U[0, 1) inputs over e4m3's range
    fp8 = torch_ext.GroupedKVCache(a.B, a.cap, dm, a.H, hk, "fa_tc_fp8", device=dev)
    fp8.set_scales(*scales)
    fp8.append(K, V)
    name = lambda w: f"window{w}"  # noqa: E731
    outs = {s: torch.empty_like(Q) for s in ["ref"] + [name(w) for w in windows]}

    def ref_call():
        _lib.check(lib.qmha_attend_cached_tokens(fp8._handle, Q.data_ptr(), outs["ref"].data_ptr(), a.nq, lens.data_ptr(), CAUSAL, stream), "attend_tokens")

    def window_call(w):
        def call():
            _lib.check(lib.qmha_attend_cached_prefill_window(fp8._handle, Q.data_ptr(), outs[name(w)].data_ptr(), a.nq, lens.data_ptr(), w,
                                                             sinks.data_ptr(), CAUSAL, stream), "attend_prefill_window")
        return call

    # ---- each candidate's O against the restatement, before anything is timed: sequence 0, the first and the last head ----
    (Qn, Kn, Vn), Sn = (x[:1].cpu().numpy() for x in (Q, K, V)), sinks.cpu().numpy()
    cols = lambda k, w: slice(k * w, (k + 1) * w)  # noqa: E731
    checks, tile_ratio = {}, {}
    dgs = [(L - a.nq) // 32 + q for q in range(-(-((L - a.nq) % 32 + a.nq) // 32))]  # the query groups' diagonal tiles
    for w in windows:
        window_call(w)()
        torch.cuda.synchronize(dev)
        got, worst = outs[name(w)][:1].cpu().numpy().astype(np.float64), 0.0
        for k in (0, a.H - 1):
            want, Ltot, vmax = ref.prefill_window(Qn[:, :, cols(k, a.d)], Kn[:, :, cols(k // G, a.d)], Vn[:, :, cols(k // G, a.d)], [L], 1, 1, scales,
                                                  a.cap, w, Sn[k:k + 1])
            bound = np.repeat(2.0 * 2.0 ** 4 * vmax[:, None, :] / Ltot, a.d, axis=-1) + 2.0 ** -16 * float(np.abs(Vn).max())
            worst = max(worst, float((np.abs(got[:, :, cols(k, a.d)] - want) / bound).max()))
        checks[name(w)] = {"finite": bool(torch.isfinite(outs[name(w)]).all()), "err_over_bound": round(worst, 4)}
        tile_ratio[name(w)] = round(sum(dg - max(0, 32 * dg - w + 1) // 32 + 1 for dg in dgs) / sum(dg + 1 for dg in dgs), 4)
    if not all(v["finite"] and v["err_over_bound"] <= 1.0 for v in checks.values()):
        print(json.dumps({"tool": "prefill_window_ab", "checks": checks}), flush=True)
        sys.exit("prefill_window_ab: a candidate's O is outside the restatement's bound")

    def batch(call, n):
        """n calls: ms per call from the library's main pairs."""
        for _ in range(n):
            call()
        torch.cuda.synchronize(dev)
        main_ms, pre_ms, k = ctypes.c_double(), ctypes.c_double(), ctypes.c_longlong()
        _lib.check(lib.qmha_profile_collect(ctypes.byref(main_ms), ctypes.byref(k), ctypes.byref(pre_ms)), "collect")
        assert k.value == n, (k.value, n)
        return main_ms.value / n

    sides = {"ref": ref_call}  # the reference first
    sides.update({name(w): window_call(w) for w in windows})
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
    med = {s: statistics.median(per[s]) for s in per}
    lo, hi = min(per["ref"]), max(per["ref"])
    res = {"tool": "prefill_window_ab", "B": a.B, "H": a.H, "h_kv": hk, "d": a.d, "cap": a.cap, "Nq": a.nq, "L": L, "rounds": a.rounds,
           "calls_per_round": a.calls, "reference": "attend_tokens", "candidate": "attend_prefill_window with sinks", "checks": checks,
           "tile_ratio_derived": tile_ratio, "ref_ms": round(med["ref"], 5), "ref_spread": round((hi - lo) / med["ref"], 4), "sides": {},
           "per_round": {s: [round(x, 5) for x in per[s]] for s in per}, "clock_probe": bench.clock_probe(dev),
           "isa_sha16": {"attend": isa_id.isa_sha16(_lib.LIB_PATH, f"qmha_fa_fp8_kernelINS_6RaggedELi{a.d}EEEv"),
                         "band": isa_id.isa_sha16(_lib.LIB_PATH, f"qmha_fp8_band_kernelINS_6RaggedELi{a.d}EEEv")},
           "device": torch.cuda.get_device_properties(dev).name}
    for s in sides:
        if s != "ref":
            # every round of the side below (a gain) / above (a loss) every round of the reference
            res["sides"][s] = {"ms": round(med[s], 5), "ratio": round(med[s] / med["ref"], 4),
                               "verdict": "gain" if max(per[s]) < lo else "loss" if min(per[s]) > hi else "inside the spread"}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
