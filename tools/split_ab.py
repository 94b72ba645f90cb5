#!/usr/bin/env python3
"""A decode step with the key sweep split into chunks (qmha_attend_cached_tokens_split) against the step
the library offered before (qmha_attend_cached_tokens), on one cache, in one process, alternating.

    python tools/split_ab.py --variant fa_tc_int8_b --B 16 --H 16 --d 64 --cap 4096 [--h-kv 4]

A cache of `cap` rows is filled once.  Sequence b holds L[b] = 32 t[b] + 17 rows, t[b] spread evenly over 512 / 32 ..
cap / 32 - 1 (B = 1: the longest), its open group built by append_tokens from the group's first row on.  Every step
appends row L[b] - 1 again (append_tokens n = 1) and attends with one query row: the reference with attend_tokens, each
candidate with attend_tokens_split at one of --chunks (default 256, 512, 1024 rows) over a scratch of its own.  The
reference sweeps up to cap / 32 key tiles with one wave per head (G waves on a grouped cache), a candidate at most
chunk_rows / 32 per workgroup, plus the combine launch.

Before anything is timed, per candidate: O is finite and non-zero; it equals the float64 evaluation of the combine formula
on the fp32 partials read back from the scratch within (2 n_c + 4) 2^-23 max|Oc|; the call over a scratch of NaN bytes and
over a zeroed one gives the same bits; two calls give the same bits; and |O - attend_tokens' O| is reported (both lie
inside the accuracy contract; they are different functions).  A miss ends the run.

With qmha_profile on, every side is warmed, then ROUNDS rounds alternate CALLS steps of each side; the figures are the
library's own event pairs (attend: one main pair around the partial and the combine launch) and a device-event pair around
each batch (the whole step, append and launches included).  Medians; the reference's round-to-round spread
(max - min) / median; a ratio counts as a gain only where every round lies outside that spread.  One JSON line.
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
    ap.add_argument("--h-kv", type=int, default=None, help="K/V heads of a grouped cache (default: H)")
    ap.add_argument("--d", type=int, default=64)
    ap.add_argument("--cap", type=int, default=4096)
    ap.add_argument("--chunks", type=int, nargs="+", default=[256, 512, 1024])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    if a.rounds < 5 or a.calls < 30:
        ap.error("at least 5 rounds of at least 30 calls")
    if a.cap % 64 or a.cap < 1024 or a.B < 1 or any(c % 64 or c < 64 or c > a.cap for c in a.chunks):
        ap.error("cap % 64 == 0, cap >= 1024, B >= 1, every chunk a multiple of 64 in [64, cap]")

    import numpy as np
    import torch
    import bench
    from quantizedmha_amd import _lib, isa_id, torch_ext
    lib = _lib.load()
    dev = torch.device("cuda:0")
    hk = a.h_kv or a.H
    dm, kvm, r = a.H * a.d, hk * a.d, 17
    g = torch.Generator(device=dev).manual_seed(a.cap + a.d)
    K, V = (torch.rand((a.B, a.cap, kvm), generator=g, device=dev, dtype=torch.float32) for _ in range(2))
    q1 = torch.rand((a.B, 1, dm), generator=g, device=dev, dtype=torch.float32)
    stream = torch.cuda.current_stream(dev).cuda_stream
    stem = "int8" if a.variant == "fa_tc_int8_b" else "f16"
    CAUSAL = _lib.QMHA_FLAG_CAUSAL
    i32 = lambda xs: torch.tensor(xs, dtype=torch.int32, device=dev)  # noqa: E731

    t0, t1 = 512 // 32, a.cap // 32 - 1
    tiles = [t1] if a.B == 1 else [t0 + round(i * (t1 - t0) / (a.B - 1)) for i in range(a.B)]
    L = [32 * t + r for t in tiles]
    rows = lambda X, first, n: torch.stack([X[b, p:p + n] for b, p in enumerate(first)]).contiguous()  # noqa: E731

    cache = (torch_ext.GroupedKVCache(a.B, a.cap, dm, a.H, hk, a.variant, device=dev) if a.h_kv
             else torch_ext.KVCache(a.B, a.cap, dm, a.H, a.variant, device=dev))
    cache.append(K, V)
    cache.enable_tokens()
    base = [32 * t for t in tiles]
    cache.append_tokens(rows(K, base, r - 1), rows(V, base, r - 1), i32(base))  # the open group, from its first row on
    k1, v1 = rows(K, [x - 1 for x in L], 1), rows(V, [x - 1 for x in L], 1)
    pos1, lens1 = i32([x - 1 for x in L]), i32(L)
    o_ref = torch.empty_like(q1)
    outs = {c: torch.empty_like(q1) for c in a.chunks}
    scratch = {c: torch.zeros(lib.qmha_attend_split_bytes(cache._handle, 1, c), dtype=torch.uint8, device=dev) for c in a.chunks}

    def append():
        _lib.check(lib.qmha_kv_cache_append_tokens(cache._handle, k1.data_ptr(), v1.data_ptr(), 1, pos1.data_ptr(), stream), "append_tokens")

    def ref_step():
        append()
        _lib.check(lib.qmha_attend_cached_tokens(cache._handle, q1.data_ptr(), o_ref.data_ptr(), 1, lens1.data_ptr(), CAUSAL, stream),
                   "attend_tokens")

    def split_step(c):
        def step():
            append()
            _lib.check(lib.qmha_attend_cached_tokens_split(cache._handle, q1.data_ptr(), outs[c].data_ptr(), 1, lens1.data_ptr(), c,
                                                           scratch[c].data_ptr(), scratch[c].numel(), CAUSAL, stream), "attend_tokens_split")
        return step

    # ---- the bit-level properties, before anything is timed ----
    ref_step()
    torch.cuda.synchronize(dev)
    want = o_ref.cpu().numpy()
    thr = 1e-20 if a.variant == "fa_tc_int8_b" else 1e-10
    checks = {}
    al = lambda x: -(-x // 256) * 256  # noqa: E731
    for c in a.chunks:
        nc = -(-a.cap // c)
        scratch[c].fill_(0xFF)  # NaN bytes
        split_step(c)()
        torch.cuda.synchronize(dev)
        over_nan = outs[c].cpu().numpy().copy()
        mem = scratch[c].cpu().numpy()
        o_bytes, s_bytes = 4 * a.B * nc * dm, 4 * a.B * nc * a.H
        Oc = mem[:o_bytes].view(np.float32).reshape(a.B, nc, a.H, a.d).astype(np.float64)
        pm = mem[al(o_bytes):al(o_bytes) + s_bytes].view(np.float32).reshape(a.B, nc, a.H).astype(np.float64)
        pl = mem[al(o_bytes) + al(s_bytes):al(o_bytes) + al(s_bytes) + s_bytes].view(np.float32).reshape(a.B, nc, a.H).astype(np.float64)
        worst = 0.0
        for b in range(a.B):
            n = (L[b] - 1) // c + 1  # the chunks the row's group reaches: its last tile is ceil32(L) / 32 - 1
            w = pl[b, :n] * np.exp2(pm[b, :n] - pm[b, :n].max(axis=0))
            tot = w.sum(axis=0)
            f64 = np.where(tot[:, None] > thr, (w[:, :, None] * Oc[b, :n]).sum(axis=0) / tot[:, None], 0.0)
            bound = (2 * n + 4) * 2.0 ** -23 * np.abs(Oc[b, :n]).max(axis=0)
            err = np.abs(over_nan[b, 0].reshape(a.H, a.d) - f64)
            worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
        scratch[c].zero_()
        split_step(c)()
        torch.cuda.synchronize(dev)
        over_zero = outs[c].cpu().numpy().copy()
        split_step(c)()
        torch.cuda.synchronize(dev)
        checks[c] = {"finite_nonzero": bool(np.isfinite(over_nan).all() and np.abs(over_nan).max() > 0.0),
                     "combine_err_over_bound": round(worst, 4),
                     "nan_scratch_same_bits": bool(np.array_equal(over_nan, over_zero)),
                     "repeat_same_bits": bool(np.array_equal(outs[c].cpu().numpy(), over_zero)),
                     "max_abs_diff_to_attend_tokens": float(np.abs(over_nan - want).max())}
    ok = all(v["finite_nonzero"] and v["combine_err_over_bound"] <= 1.0 and v["nan_scratch_same_bits"] and v["repeat_same_bits"]
             for v in checks.values())
    if not ok:
        print(json.dumps({"tool": "split_ab", "checks": checks}), flush=True)
        sys.exit("split_ab: a bit-level property of the split call does not hold")

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
    sides.update({f"split{c}": split_step(c) for c in a.chunks})
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
    res = {"tool": "split_ab", "variant": a.variant, "B": a.B, "H": a.H, "h_kv": hk, "d": a.d, "cap": a.cap, "lens": L,
           "rounds": a.rounds, "calls_per_round": a.calls, "reference": "append_tokens n=1 + attend_tokens Nq=1",
           "candidate": "append_tokens n=1 + attend_tokens_split Nq=1 (partial + combine)", "checks": checks,
           "ref_attend_ms": round(med["ref"][0], 5), "ref_step_ms": round(med["ref"][2], 5), "append_ms": round(med["ref"][1], 5),
           "ref_attend_spread": round(spread(ref_main, med["ref"][0]), 4), "ref_step_spread": round(spread(ref_step_ms, med["ref"][2]), 4),
           "split": {}, "per_round": {s: [[round(x, 5) for x in row] for row in per[s]] for s in per},
           "clock_probe": bench.clock_probe(dev),
           "isa_sha16": {"ragged_main": isa_id.isa_sha16(_lib.LIB_PATH, f"qmha_fa_{stem}_cache_kernelILi{a.d}ENS_6RaggedEEEv"),
                         "split_main": isa_id.isa_sha16(_lib.LIB_PATH, f"qmha_fa_{stem}_split_kernelILi{a.d}ENS_6Ragged"),
                         "combine": isa_id.isa_sha16(_lib.LIB_PATH, "qmha_split_combine_kernel")},
           "device": torch.cuda.get_device_properties(dev).name}
    lo_main, hi_main = min(ref_main), max(ref_main)
    lo_step, hi_step = min(ref_step_ms), max(ref_step_ms)
    for c in a.chunks:
        s = f"split{c}"
        res["split"][str(c)] = {
            "attend_ms": round(med[s][0], 5), "step_ms": round(med[s][2], 5),
            "attend_ratio": round(med[s][0] / med["ref"][0], 4), "step_ratio": round(med[s][2] / med["ref"][2], 4),
            # every round of the candidate below (a gain) / above (a loss) every round of the reference
            "attend_verdict": "gain" if max(x[0] for x in per[s]) < lo_main else "loss" if min(x[0] for x in per[s]) > hi_main else "inside the spread",
            "step_verdict": "gain" if max(x[2] for x in per[s]) < lo_step else "loss" if min(x[2] for x in per[s]) > hi_step else "inside the spread"}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
