#!/usr/bin/env python3
"""A decode step (qmha_kv_cache_append_tokens n = 1 plus qmha_attend_cached_tokens Nq = 1) and one prefill chunk (Nq = 1024
at L = cap) on an e4m3 cache (fa_tc_fp8) against the same calls on an fp16 and an int8 cache, in one process,
alternating.

    python tools/fp8_ab.py --B 16 --H 16 --d 64 --cap 4096

Three caches of `cap` rows are filled once; sequence b holds L[b] = 32 t[b] + 17 rows, t[b] spread evenly over 512 / 32 ..
cap / 32 - 1, the open group built by append_tokens from its first row on.  Before anything is timed the fp8 cache's O of
the decode step is held to the contract's restatement (tests/fp8_ref.py) for sequence 0, head 0.  With qmha_profile on,
all sides are warmed, then ROUNDS rounds alternate CALLS steps of each side, the fp16 reference first; the figures are the
library's own event pairs (append: pre-pass, attend: main kernel).  The yardstick of a ratio is the fp16 reference's own
round-to-round spread.  One JSON line."""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SIDES = ["fa_tc_v1a", "fa_tc_int8_b", "fa_tc_fp8"]  # the reference first


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=16)
    ap.add_argument("--H", type=int, default=16)
    ap.add_argument("--d", type=int, default=64)
    ap.add_argument("--cap", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    if a.rounds < 5 or a.calls < 30 or a.cap % 32 or a.cap < 1024 or a.B < 2:
        ap.error("at least 5 rounds of at least 30 calls; cap % 32 == 0, cap >= 1024, B >= 2")

    import numpy as np
    import torch
    import bench
    from quantizedmha_amd import _lib, torch_ext
    from tests import fp8_ref
    lib = _lib.load()
    dev = torch.device("cuda:0")
    dm, r, NP = a.H * a.d, 17, 1024
    g = torch.Generator(device=dev).manual_seed(a.cap + a.d)
    K, V = (torch.rand((a.B, a.cap, dm), generator=g, device=dev, dtype=torch.float32) for _ in range(2))
    Q = torch.rand((a.B, NP, dm), generator=g, device=dev, dtype=torch.float32)
    i32 = lambda xs: torch.tensor(xs, dtype=torch.int32, device=dev)  # noqa: E731
    t0, t1 = 512 // 32, a.cap // 32 - 1
    L = [32 * (t0 + round(i * (t1 - t0) / (a.B - 1))) + r for i in range(a.B)]
    rows = lambda X, first, n: torch.stack([X[b, p:p + n] for b, p in enumerate(first)]).contiguous()  # noqa: E731
    k1, v1, q1 = rows(K, [x - 1 for x in L], 1), rows(V, [x - 1 for x in L], 1), Q[:, :1].contiguous()
    pos1, lens1, full = i32([x - 1 for x in L]), i32(L), i32([a.cap] * a.B)

    caches, steps = {}, {}
    for s in SIDES:
        c = caches[s] = torch_ext.KVCache(a.B, a.cap, dm, a.H, s, device=dev)
        c.enable_tokens()
        c.append_tokens(K, V, i32([0] * a.B))  # every row, so the prefill chunk has its keys; the decode step rewrites row L - 1
        o1, op = torch.empty_like(q1), torch.empty_like(Q)

        def decode(c=c, o1=o1):
            c.append_tokens(k1, v1, pos1)
            c.attend_tokens(q1, lens1, out=o1.view(-1))

        steps[s + " decode"], steps[s + " prefill"] = decode, (lambda c=c, op=op: c.attend_tokens(Q, full, out=op.view(-1)))
        if s == "fa_tc_fp8":  # O before timing
            decode()
            torch.cuda.synchronize(dev)
            kb, vb = (X[0, :L[0], :a.d].cpu().numpy() for X in (K, V))
            k8, _, v8 = fp8_ref.cache_arrays(kb, vb, L[0], 1.0, 1.0)
            ops = [fp8_ref.decode(x) for x in (fp8_ref.encode(q1[0, :, :a.d].cpu().numpy(), 1.0), k8, v8)]
            want, l, vmax = fp8_ref.attend(*ops, L[0], (1.0, 1.0, 1.0))
            err = float(np.abs(o1[0, :, :a.d].cpu().numpy() - want).max())
            ok = err <= 2.0 * 16.0 * vmax / float(l.min()) + 2.0 ** -12  # two one-flip units and L * 2^-24 for fp32

    def batch(call, n, records):
        for _ in range(n):
            call()
        torch.cuda.synchronize(dev)
        main_ms, pre_ms, k = ctypes.c_double(), ctypes.c_double(), ctypes.c_longlong()
        _lib.check(lib.qmha_profile_collect(ctypes.byref(main_ms), ctypes.byref(k), ctypes.byref(pre_ms)), "collect")
        assert k.value == records * n, (k.value, n)
        return main_ms.value / n, pre_ms.value / n

    lib.qmha_profile_collect(None, None, None)
    lib.qmha_profile_enable(1)
    try:
        per = {s: [] for s in steps}
        for s, call in steps.items():
            batch(call, a.warmup, 2 if "decode" in s else 1)
        for _ in range(a.rounds):
            for s, call in steps.items():
                per[s].append(batch(call, a.calls, 2 if "decode" in s else 1))
    finally:
        lib.qmha_profile_enable(0)
    med = {s: [statistics.median(x[i] for x in per[s]) for i in range(2)] for s in per}
    spread = {k: (max(x[0] for x in per[f"fa_tc_v1a {k}"]) - min(x[0] for x in per[f"fa_tc_v1a {k}"])) / med[f"fa_tc_v1a {k}"][0]
              for k in ("decode", "prefill")}
    res = {"tool": "fp8_ab", "B": a.B, "H": a.H, "d": a.d, "cap": a.cap, "lens": L, "prefill_nq": NP, "rounds": a.rounds,
           "calls_per_round": a.calls, "fp8_decode_o_max_err": err, "fp8_decode_o_within_contract": bool(ok),
           "cache_bytes": {s: caches[s].mem.numel() for s in SIDES},
           "main_kernel_ms": {s: round(m[0], 5) for s, m in med.items()}, "append_ms": {s: round(m[1], 5) for s, m in med.items() if "decode" in s},
           "fp8_over_fp16_main": {k: round(med[f"fa_tc_fp8 {k}"][0] / med[f"fa_tc_v1a {k}"][0], 4) for k in spread},
           "fp16_main_spread": {k: round(v, 4) for k, v in spread.items()},
           "per_round": {s: [[round(x, 5) for x in row] for row in per[s]] for s in per},
           "clock_probe": bench.clock_probe(dev), "device": torch.cuda.get_device_properties(dev).name}
    print(json.dumps(res), flush=True)
    if not ok:
        sys.exit("fp8_ab: the fp8 cache's O is outside the contract's bound")


if __name__ == "__main__":
    main()
