#!/usr/bin/env python3
"""A decode step of a paged fp8 cache whose sequences share a prefix, through the shared-prefix decode call
(qmha_attend_cached_paged_decode_shared) against the step the library offered before: attend_paged_decode at the
same chunk_rows on the same pool, whose tables alias the prefix pages.  One process, alternating.

    python tools/shared_ab.py --B 16 --H 16 --d 64 --cap 4096 --prefix 2048 [--h-kv 4]

Sequence b holds L[b] = prefix + 32 t[b] + 17 rows, t[b] spread evenly over 0 .. (cap - prefix) / 32 - 1 (B = 1: the longest);
one query row per sequence.  Only the attend launches are timed (the library's own event pair around the partial and the
combine launch); nothing is appended between calls.  Before anything is timed the candidate's O must equal the reference's bit
for bit; a miss ends the run.  Then every side is warmed and ROUNDS rounds alternate CALLS calls of each side.  Medians; the
reference's round-to-round spread (max - min) / median; a ratio counts as a gain only where every round lies below every round
of the reference.  Beside each ratio the tile ratio R = (prefix tiles * column groups + sum_b suffix tiles_b) / sum_b tiles_b,
which ignores the combine and the launches.  One JSON line.
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
    ap.add_argument("--prefix", type=int, default=2048)
    ap.add_argument("--page-rows", type=int, default=256)
    ap.add_argument("--chunks", type=int, nargs="+", default=[256, 512, 1024])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    if a.rounds < 5 or a.calls < 30:
        ap.error("at least 5 rounds of at least 30 calls")

    import torch
    import bench
    from quantizedmha_amd import _lib, isa_id, torch_ext
    lib = _lib.load()
    dev = torch.device("cuda:0")
    hk = a.h_kv or a.H
    dm, kvm, P, pr = a.H * a.d, hk * a.d, a.prefix, a.page_rows
    g = torch.Generator(device=dev).manual_seed(a.cap + a.d)
    K, V = (torch.rand((a.B, a.cap, kvm), generator=g, device=dev, dtype=torch.float32) for _ in range(2))
    q1 = torch.rand((a.B, 1, dm), generator=g, device=dev, dtype=torch.float32)
    stream = torch.cuda.current_stream(dev).cuda_stream
    CAUSAL = _lib.QMHA_FLAG_CAUSAL
    i32 = lambda xs: torch.tensor(xs, dtype=torch.int32, device=dev)  # noqa: E731

    t1 = (a.cap - P) // 32 - 1
    tiles = [t1] if a.B == 1 else [round(i * t1 / (a.B - 1)) for i in range(a.B)]
    L = [P + 32 * t + 17 for t in tiles]
    # the pool: the prefix's pages once, then every sequence's own pages from row `prefix` on; every table aliases the prefix
    pp, mp = P // pr, a.cap // pr
    table = i32([list(range(pp)) + [pp + b * (mp - pp) + j for j in range(mp - pp)] for b in range(a.B)])
    cache = torch_ext.PagedKVCache(a.B, pp + a.B * (mp - pp), pr, mp, dm, a.H, hk, "fa_tc_fp8", str(dev))
    cache.set_scales(1.0 / 256, 1.0 / 256, 1.0 / 256)  # U[0, 1) inputs over e4m3's range
    cache.enable_tokens()
    for b in range(a.B):
        lo = P if b else 0
        Kn, Vn = (x[0 if lo == 0 else b, lo:L[b]].expand(a.B, -1, -1).contiguous() for x in (K, V))
        cache.append_paged(Kn, Vn, i32([lo if i == b else -1 for i in range(a.B)]), table)
    lens1 = i32(L)
    scr = {c: torch.zeros(lib.qmha_attend_decode_bytes(cache._handle, 1, c), dtype=torch.uint8, device=dev) for c in a.chunks}
    outs = {s: torch.empty_like(q1) for c in a.chunks for s in (f"ref{c}", f"shared{c}")}

    def ref_call(c):
        return lambda: _lib.check(lib.qmha_attend_cached_paged_decode(cache._handle, q1.data_ptr(), outs[f"ref{c}"].data_ptr(), 1, lens1.data_ptr(),
                                                                      table.data_ptr(), c, scr[c].data_ptr(), scr[c].numel(), CAUSAL, stream),
                                  "attend_paged_decode")

    def shared_call(c):
        return lambda: _lib.check(lib.qmha_attend_cached_paged_decode_shared(cache._handle, q1.data_ptr(), outs[f"shared{c}"].data_ptr(), 1,
                                                                             lens1.data_ptr(), table.data_ptr(), P, c, scr[c].data_ptr(),
                                                                             scr[c].numel(), CAUSAL, stream), "attend_paged_decode_shared")

    sides = {}
    for c in a.chunks:  # each reference ahead of its candidate
        sides[f"ref{c}"], sides[f"shared{c}"] = ref_call(c), shared_call(c)
    # ---- the candidate's bits against the reference's, before anything is timed ----
    for call in sides.values():
        call()
    torch.cuda.synchronize(dev)
    checks = {c: bool(torch.equal(outs[f"ref{c}"].view(torch.int32), outs[f"shared{c}"].view(torch.int32))) and
              bool(torch.isfinite(outs[f"ref{c}"]).all()) and bool((outs[f"ref{c}"] != 0).any()) for c in a.chunks}
    if not all(checks.values()):
        print(json.dumps({"tool": "shared_ab", "bits_equal": checks}), flush=True)
        sys.exit("shared_ab: the shared call's O is not the reference's")

    def batch(call, n):
        """n calls: attend ms per call from the library's main pairs."""
        for _ in range(n):
            call()
        torch.cuda.synchronize(dev)
        main_ms, pre_ms, k = ctypes.c_double(), ctypes.c_double(), ctypes.c_longlong()
        _lib.check(lib.qmha_profile_collect(ctypes.byref(main_ms), ctypes.byref(k), ctypes.byref(pre_ms)), "collect")
        assert k.value == n, (k.value, n)
        return main_ms.value / n

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
    W = a.H // hk
    blocks = -(-a.B * W // 16)
    qbp = 2 if blocks > 1 else 1
    groups, all_tiles = -(-blocks // qbp), sum(-(-x // 32) for x in L)
    R = (P // 32 * groups + all_tiles - a.B * (P // 32)) / all_tiles
    res = {"tool": "shared_ab", "B": a.B, "H": a.H, "h_kv": hk, "d": a.d, "cap": a.cap, "prefix_rows": P, "page_rows": pr, "lens": L,
           "rounds": a.rounds, "calls_per_round": a.calls, "reference": "attend_paged_decode Nq=1, tables alias the prefix pages",
           "candidate": "attend_paged_decode_shared Nq=1 (prefix + suffix items, combine)", "bits_equal": checks,
           "tile_ratio_R": round(R, 4), "yardstick_1.2R": round(1.2 * R, 4), "column_groups": groups, "sides": {},
           "per_round_ms": {s: [round(x, 5) for x in per[s]] for s in per}, "clock_probe": bench.clock_probe(dev),
           "isa_sha16": {"shared": isa_id.isa_sha16(_lib.LIB_PATH, f"qmha_fp8_shared_kernelINS_5PagedELi{a.d}ELi{qbp}ELi{2 if W > 16 else 1}EEEv"),
                         "decode": isa_id.isa_sha16(_lib.LIB_PATH, f"qmha_fp8_decode_kernelINS_5PagedELi{a.d}ELi{2 if W > 16 else 1}EEEv")},
           "device": torch.cuda.get_device_properties(dev).name}
    for c in a.chunks:
        ref, got = per[f"ref{c}"], per[f"shared{c}"]
        mr, mg = statistics.median(ref), statistics.median(got)
        res["sides"][f"chunk{c}"] = {
            "ref_ms": round(mr, 5), "shared_ms": round(mg, 5), "ratio": round(mg / mr, 4), "ref_spread": round((max(ref) - min(ref)) / mr, 4),
            # every round of the candidate below (a gain) / above (a loss) every round of the reference
            "verdict": "gain" if max(got) < min(ref) else "loss" if min(got) > max(ref) else "inside the spread",
            "within_1.2R": bool(mg / mr <= 1.2 * R)}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
