#!/usr/bin/env python3
"""A decode step under a sliding window (qmha_attend_cached_tokens_window) against the full-causal step
(qmha_attend_cached_tokens), on one cache, in one process, alternating; and one prefill chunk the same way.

    python tools/window_ab.py --variant fa_tc_int8_b --B 16 --H 16 --d 64 --cap 4096

A cache of `cap` rows is filled once.  Sequence b holds L[b] = 32 t[b] + 17 rows, t[b] spread evenly over 512 / 32 ..
cap / 32 - 1 (B = 1: the longest), its open group built by append_tokens from the group's first row on.  Every step
appends row L[b] - 1 again (append_tokens n = 1) and attends with one query row: the reference with attend_tokens, each
candidate with attend_tokens_window at one of --windows (default 256, 1024, cap rows).  The reference sweeps
GL[b] = ceil32(L[b]) / 32 key tiles with one wave per head, a candidate min(window / 32 + 1, GL[b]).  The prefill chunk is
Nq = --prefill-nq rows (default 1024) at L = cap under --prefill-window (default 1024), attends only.

Before anything is timed, per candidate: O is finite and lies within the accuracy contract (int8 5e-3, fp16
max(1e-3, 1e-3 |ref|)) of float64 band attention over the raw rows; two calls give the same bits; and a window >= cap gives
attend_tokens' bits.  A miss ends the run.

With qmha_profile on, every side is warmed, then ROUNDS rounds alternate CALLS steps of each side; the figures are the
library's own event pairs (attend: the main pair) and a device-event pair around each batch (the whole step).  Medians; the
reference's round-to-round spread (max - min) / median.  Each ratio stands beside the tile ratio R expected from the tile
counts alone and the project's 1.2 R yardstick (README).  One JSON line.
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
    ap.add_argument("--windows", type=int, nargs="+", default=None)
    ap.add_argument("--prefill-nq", type=int, default=1024)
    ap.add_argument("--prefill-window", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    windows = a.windows or [256, 1024, a.cap]
    if a.rounds < 5 or a.calls < 30:
        ap.error("at least 5 rounds of at least 30 calls")
    if a.cap % 64 or a.cap < 1024 or a.B < 1 or any(w % 32 or w < 32 for w in windows + [a.prefill_window]) or not 1 <= a.prefill_nq <= a.cap:
        ap.error("cap % 64 == 0, cap >= 1024, B >= 1, every window a multiple of 32 >= 32, 1 <= prefill-nq <= cap")

    import numpy as np
    import torch
    import bench
    from quantizedmha_amd import _lib, isa_id, torch_ext
    lib = _lib.load()
    dev = torch.device("cuda:0")
    dm, r = a.H * a.d, 17
    g = torch.Generator(device=dev).manual_seed(a.cap + a.d)
    K, V = (torch.rand((a.B, a.cap, dm), generator=g, device=dev, dtype=torch.float32) for _ in range(2))
    q1 = torch.rand((a.B, 1, dm), generator=g, device=dev, dtype=torch.float32)
    qp = torch.rand((a.B, a.prefill_nq, dm), generator=g, device=dev, dtype=torch.float32)
    stream = torch.cuda.current_stream(dev).cuda_stream
    stem = "int8" if a.variant == "fa_tc_int8_b" else "f16"
    CAUSAL = _lib.QMHA_FLAG_CAUSAL
    i32 = lambda xs: torch.tensor(xs, dtype=torch.int32, device=dev)  # noqa: E731

    t0, t1 = 512 // 32, a.cap // 32 - 1
    tiles = [t1] if a.B == 1 else [t0 + round(i * (t1 - t0) / (a.B - 1)) for i in range(a.B)]
    L = [32 * t + r for t in tiles]
    GL = [t + 1 for t in tiles]
    rows = lambda X, first, n: torch.stack([X[b, p:p + n] for b, p in enumerate(first)]).contiguous()  # noqa: E731

    def build_cache():
        c = torch_ext.KVCache(a.B, a.cap, dm, a.H, a.variant, device=dev)
        c.append(K, V)
        c.enable_tokens()
        return c

    cache = build_cache()
    base = [32 * t for t in tiles]
    cache.append_tokens(rows(K, base, r - 1), rows(V, base, r - 1), i32(base))  # the open group, from its first row on
    k1, v1 = rows(K, [x - 1 for x in L], 1), rows(V, [x - 1 for x in L], 1)
    pos1, lens1 = i32([x - 1 for x in L]), i32(L)
    full = build_cache()  # the prefill chunk's: all cap rows
    lens_full = i32([a.cap] * a.B)
    o_ref, op_ref, op_win = torch.empty_like(q1), torch.empty_like(qp), torch.empty_like(qp)
    outs = {w: torch.empty_like(q1) for w in windows}

    def append():
        _lib.check(lib.qmha_kv_cache_append_tokens(cache._handle, k1.data_ptr(), v1.data_ptr(), 1, pos1.data_ptr(), stream), "append_tokens")

    def attend(c, q, o, lens, window):
        if window is None:
            st = lib.qmha_attend_cached_tokens(c._handle, q.data_ptr(), o.data_ptr(), q.shape[1], lens.data_ptr(), CAUSAL, stream)
        else:
            st = lib.qmha_attend_cached_tokens_window(c._handle, q.data_ptr(), o.data_ptr(), q.shape[1], lens.data_ptr(), window, CAUSAL, stream)
        _lib.check(st, "attend_tokens" if window is None else "attend_tokens_window")

    def decode_step(window):
        def step():
            append()
            attend(cache, q1, o_ref if window is None else outs[window], lens1, window)
        return step

    def prefill(window):
        return lambda: attend(full, qp, op_ref if window is None else op_win, lens_full, window)

    def band_f64(q, Lb, b, window):
        """float64 band attention of rows q [Nq, dm] of sequence b over its first Lb rows."""
        Kb, Vb = K[b, :Lb].cpu().numpy().astype(np.float64), V[b, :Lb].cpu().numpy().astype(np.float64)
        q = q.cpu().numpy().astype(np.float64)
        Nq = q.shape[0]
        pos = np.arange(Nq)[:, None] + (Lb - Nq)
        j = np.arange(Lb)[None, :]
        hidden = (j > pos) | (j <= pos - window)
        out = np.zeros_like(q)
        for k in range(a.H):
            sl = slice(k * a.d, (k + 1) * a.d)
            s = np.where(hidden, -np.inf, q[:, sl] @ Kb[:, sl].T / np.sqrt(a.d))
            p = np.exp(s - s.max(-1, keepdims=True))
            out[:, sl] = (p / p.sum(-1, keepdims=True)) @ Vb[:, sl]
        return out

    def inside(got, ref):
        err = np.abs(got.astype(np.float64) - ref)
        ok = (err <= 5e-3) if a.variant == "fa_tc_int8_b" else (err <= np.maximum(1e-3, 1e-3 * np.abs(ref)))
        return bool(np.isfinite(got).all() and ok.all()), float(err.max())

    # ---- the checks, before anything is timed ----
    decode_step(None)()
    torch.cuda.synchronize(dev)
    want = o_ref.cpu().numpy()
    checks = {}
    for w in windows:
        decode_step(w)()
        torch.cuda.synchronize(dev)
        first = outs[w].cpu().numpy().copy()
        decode_step(w)()
        torch.cuda.synchronize(dev)
        verdicts = [inside(first[b], band_f64(q1[b], L[b], b, w)) for b in range(a.B)]
        checks[str(w)] = {"within_contract_of_float64": all(v[0] for v in verdicts), "max_err_to_float64": max(v[1] for v in verdicts),
                          "nonzero": bool(np.abs(first).max() > 0.0), "repeat_same_bits": bool(np.array_equal(outs[w].cpu().numpy(), first))}
        if w >= a.cap:
            checks[str(w)]["attend_tokens_bits"] = bool(np.array_equal(first, want))
    prefill(None)(), prefill(a.prefill_window)()
    torch.cuda.synchronize(dev)
    pv = [inside(op_win[b].cpu().numpy(), band_f64(qp[b], a.cap, b, a.prefill_window)) for b in range(min(a.B, 2))]
    checks["prefill"] = {"within_contract_of_float64": all(v[0] for v in pv), "max_err_to_float64": max(v[1] for v in pv),
                         "sequences_checked": len(pv)}
    if not all(all(v for k, v in c.items() if isinstance(v, bool)) for c in checks.values()):
        print(json.dumps({"tool": "window_ab", "checks": checks}), flush=True)
        sys.exit("window_ab: a property of the windowed call does not hold")

    def batch(call, n, records):
        """n calls: (attend ms from the library's main pairs, append ms, wall ms between device events) per call."""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            call()
        e1.record()
        torch.cuda.synchronize(dev)
        main_ms, pre_ms, k = ctypes.c_double(), ctypes.c_double(), ctypes.c_longlong()
        _lib.check(lib.qmha_profile_collect(ctypes.byref(main_ms), ctypes.byref(k), ctypes.byref(pre_ms)), "collect")
        assert k.value == records * n, (k.value, n)
        return main_ms.value / n, pre_ms.value / n, e0.elapsed_time(e1) / n

    def alternate(sides, records):
        for call in sides.values():
            batch(call, a.warmup, records)
        per = {s: [] for s in sides}
        for _ in range(a.rounds):
            for s, call in sides.items():
                per[s].append(batch(call, a.calls, records))
        return per

    decode = {"ref": decode_step(None)}  # the reference first
    decode.update({f"window{w}": decode_step(w) for w in windows})
    chunk = {"ref": prefill(None), "window": prefill(a.prefill_window)}
    lib.qmha_profile_collect(None, None, None)
    lib.qmha_profile_enable(1)
    try:
        per = alternate(decode, 2)  # one record per append, one per attend
        per_p = alternate(chunk, 1)
    finally:
        lib.qmha_profile_enable(0)
    med = lambda rows_, i: statistics.median(x[i] for x in rows_)  # noqa: E731
    spread = lambda rows_, i: (max(x[i] for x in rows_) - min(x[i] for x in rows_)) / med(rows_, i)  # noqa: E731

    def verdict(cand, ref, i):
        return "gain" if max(x[i] for x in cand) < min(x[i] for x in ref) else "loss" if min(x[i] for x in cand) > max(x[i] for x in ref) else "inside the spread"

    res = {"tool": "window_ab", "variant": a.variant, "B": a.B, "H": a.H, "d": a.d, "cap": a.cap, "lens": L, "rounds": a.rounds,
           "calls_per_round": a.calls, "reference": "append_tokens n=1 + attend_tokens Nq=1",
           "candidate": "append_tokens n=1 + attend_tokens_window Nq=1", "checks": checks,
           "ref_attend_ms": round(med(per["ref"], 0), 5), "ref_step_ms": round(med(per["ref"], 2), 5), "append_ms": round(med(per["ref"], 1), 5),
           "ref_attend_spread": round(spread(per["ref"], 0), 4), "ref_step_spread": round(spread(per["ref"], 2), 4), "window": {},
           "per_round": {s: [[round(x, 5) for x in row] for row in per[s]] for s in per}}
    for w in windows:
        s = f"window{w}"
        R = sum(min(w // 32 + 1, gl) for gl in GL) / sum(GL)
        ratio = med(per[s], 0) / med(per["ref"], 0)
        res["window"][str(w)] = {"attend_ms": round(med(per[s], 0), 5), "step_ms": round(med(per[s], 2), 5), "attend_ratio": round(ratio, 4),
                                 "step_ratio": round(med(per[s], 2) / med(per["ref"], 2), 4), "tile_ratio_R": round(R, 4),
                                 "yardstick_1.2R": round(1.2 * R, 4), "within_yardstick": bool(ratio <= 1.2 * R),
                                 "attend_verdict": verdict(per[s], per["ref"], 0), "step_verdict": verdict(per[s], per["ref"], 2)}
    # the prefill chunk: query group qg of Nq / 32 (L = cap, s = 0) sweeps diag + 1 tiles, diag = qg + (cap - Nq) / 32
    wp, off = a.prefill_window // 32, (a.cap - -(-a.prefill_nq // 32) * 32) // 32
    groups = -(-a.prefill_nq // 32)
    Rp = sum(min(wp + 1, qg + off + 1) for qg in range(groups)) / sum(qg + off + 1 for qg in range(groups))
    ratio_p = med(per_p["window"], 0) / med(per_p["ref"], 0)
    res["prefill"] = {"Nq": a.prefill_nq, "L": a.cap, "window": a.prefill_window, "ref_attend_ms": round(med(per_p["ref"], 0), 5),
                      "attend_ms": round(med(per_p["window"], 0), 5), "attend_ratio": round(ratio_p, 4),
                      "ref_attend_spread": round(spread(per_p["ref"], 0), 4), "tile_ratio_R": round(Rp, 4), "yardstick_1.2R": round(1.2 * Rp, 4),
                      "within_yardstick": bool(ratio_p <= 1.2 * Rp), "attend_verdict": verdict(per_p["window"], per_p["ref"], 0),
                      "per_round": {s: [[round(x, 5) for x in row] for row in per_p[s]] for s in per_p}}
    res["clock_probe"] = bench.clock_probe(dev)
    res["isa_sha16"] = {"ragged_main": isa_id.isa_sha16(_lib.LIB_PATH, f"qmha_fa_{stem}_cache_kernelILi{a.d}ENS_6RaggedEEEv"),
                        "window_main": isa_id.isa_sha16(_lib.LIB_PATH, f"qmha_fa_{stem}_window_kernelINS_6RaggedELi{a.d}EEEv")}
    res["device"] = torch.cuda.get_device_properties(dev).name
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
