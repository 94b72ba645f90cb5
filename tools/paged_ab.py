#!/usr/bin/env python3
"""A decode step through a paged cache (qmha_kv_cache_append_paged n = 1 plus qmha_attend_cached_paged Nq = 1)
against the same step on a contiguous cache (qmha_kv_cache_append_tokens plus qmha_attend_cached_tokens), in one process,
alternating.

    python tools/paged_ab.py --variant fa_tc_int8_b --B 16 --H 16 --d 64 --cap 4096

Sequence b holds L[b] = 32 t[b] + 17 rows, t[b] spread evenly over 16 .. 127 (one n per call).  The contiguous cache of
`cap` rows and, for each page size (64 and 256 rows), a pool of B cap / page_rows pages under a randomly permuted table
are filled with the same rows, the open group built token-wise from its first row on.  A step appends row L[b] - 1 again
and attends with one query row: both sides visit the same key tiles with the same arithmetic, so the main-kernel ratio
is expected near 1; what the paged kernels add is one table load and one descriptor rebuild per stage.  With
qmha_profile on, every side is warmed, then ROUNDS rounds alternate CALLS steps of the reference and of each paged side;
the figures are the library's own event pairs (append: pre-pass, attend: main kernel) and a device-event pair around
each batch (the whole step, launches included).  Every paged O is compared bit for bit with the contiguous one before
anything is timed.  One JSON line, with the pool's bytes against the contiguous cache's for a batch whose lengths
spread over 512 .. cap (host arithmetic).
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PAGE_SIZES = (64, 256)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variant", default="fa_tc_int8_b", choices=["fa_tc_int8_b", "fa_tc_v1a"])
    ap.add_argument("--B", type=int, default=16)
    ap.add_argument("--H", type=int, default=16)
    ap.add_argument("--d", type=int, default=64)
    ap.add_argument("--cap", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    if a.rounds < 5 or a.calls < 30:
        ap.error("at least 5 rounds of at least 30 calls")
    if a.cap % 256 or a.cap < 4096 or a.B < 2:
        ap.error("cap % 256 == 0, cap >= 4096, B >= 2")

    import torch
    import bench
    from quantizedmha_amd import _lib, isa_id, torch_ext
    lib = _lib.load()
    dev = torch.device("cuda:0")
    dm, r = a.H * a.d, 17
    g = torch.Generator(device=dev).manual_seed(a.cap + a.d)
    K, V = (torch.rand((a.B, a.cap, dm), generator=g, device=dev, dtype=torch.float32) for _ in range(2))
    Q = torch.rand((a.B, 1, dm), generator=g, device=dev, dtype=torch.float32)
    stream = torch.cuda.current_stream(dev).cuda_stream
    stem = "int8" if a.variant == "fa_tc_int8_b" else "f16"
    CAUSAL = _lib.QMHA_FLAG_CAUSAL
    i32 = lambda xs: torch.tensor(xs, dtype=torch.int32, device=dev)  # noqa: E731

    t0, t1 = 16, 127
    tiles = [t0 + round(i * (t1 - t0) / (a.B - 1)) for i in range(a.B)]
    L = [32 * t + r for t in tiles]
    rows = lambda X, first, n: torch.stack([X[b, p:p + n] for b, p in enumerate(first)]).contiguous()  # noqa: E731
    base = [32 * t for t in tiles]
    k1, v1 = rows(K, [x - 1 for x in L], 1), rows(V, [x - 1 for x in L], 1)
    pos1, lens1 = i32([x - 1 for x in L]), i32(L)

    def fill(append):
        """Whole groups in one call per sequence (the lengths differ), then the open group from its first row on."""
        for b in range(a.B):
            pos = [0 if i == b else -1 for i in range(a.B)]
            n = base[b]
            append(rows(K, [0] * a.B, n), rows(V, [0] * a.B, n), i32(pos))
        append(rows(K, base, r - 1), rows(V, base, r - 1), i32(base))

    ref = torch_ext.KVCache(a.B, a.cap, dm, a.H, a.variant, device=dev)
    ref.enable_tokens()
    fill(ref.append_tokens)
    o_ref = torch.empty_like(Q)

    def ref_step():
        _lib.check(lib.qmha_kv_cache_append_tokens(ref._handle, k1.data_ptr(), v1.data_ptr(), 1, pos1.data_ptr(), stream), "append_tokens")
        _lib.check(lib.qmha_attend_cached_tokens(ref._handle, Q.data_ptr(), o_ref.data_ptr(), 1, lens1.data_ptr(), CAUSAL, stream),
                   "attend_tokens")

    sides = {"contiguous": ref_step}  # the reference first
    outs, pools = {}, {}
    for pr in PAGE_SIZES:
        mp = a.cap // pr
        perm = torch.randperm(a.B * mp, generator=torch.Generator().manual_seed(pr)).to(torch.int32)
        table = perm.view(a.B, mp).contiguous().to(dev)
        pool = torch_ext.PagedKVCache(a.B, a.B * mp, pr, mp, dm, a.H, None, a.variant, device=dev)
        pool.enable_tokens()
        fill(lambda k, v, p, pool=pool, table=table: pool.append_paged(k, v, p, table))
        o = torch.empty_like(Q)

        def step(pool=pool, table=table, o=o):
            _lib.check(lib.qmha_kv_cache_append_paged(pool._handle, k1.data_ptr(), v1.data_ptr(), 1, pos1.data_ptr(), table.data_ptr(),
                                                      stream), "append_paged")
            _lib.check(lib.qmha_attend_cached_paged(pool._handle, Q.data_ptr(), o.data_ptr(), 1, lens1.data_ptr(), table.data_ptr(),
                                                    CAUSAL, stream), "attend_paged")

        sides[f"paged{pr}"] = step
        outs[f"paged{pr}"], pools[f"paged{pr}"] = o, pool

    # O before timing: every paged side against the contiguous step
    for call in sides.values():
        call()
    torch.cuda.synchronize(dev)
    same = {s: bool(torch.equal(o, o_ref)) for s, o in outs.items()}
    sane = bool(torch.isfinite(o_ref).all()) and float(o_ref.abs().max()) > 0.0

    def batch(call, n):
        """n steps: (main-kernel ms, pre-pass ms, whole-step ms) per step."""
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
    names = ("main_kernel", "append", "step")
    spread = [(max(x[i] for x in per["contiguous"]) - min(x[i] for x in per["contiguous"])) / med["contiguous"][i] for i in range(3)]

    # memory, host arithmetic: a batch whose lengths spread evenly over 512 .. cap, pages taken as the rows need them
    vid = _lib.variant_id(a.variant)
    spread_lens = [512 + round(i * (a.cap - 512) / (a.B - 1)) for i in range(a.B)]
    contiguous_bytes = lib.qmha_kv_cache_bytes(a.B, a.cap, dm, a.H, vid)
    memory = {"lens": spread_lens, "contiguous_bytes": contiguous_bytes}
    for pr in PAGE_SIZES:
        pages = sum(-(-x // pr) for x in spread_lens)
        memory[f"paged{pr}_pages"] = pages
        memory[f"paged{pr}_bytes"] = lib.qmha_kv_cache_paged_bytes(pages, pr, dm, a.H, a.H, vid)
        memory[f"paged{pr}_share"] = round(memory[f"paged{pr}_bytes"] / contiguous_bytes, 4)

    res = {"tool": "paged_ab", "variant": a.variant, "B": a.B, "H": a.H, "d": a.d, "cap": a.cap, "lens": L,
           "rounds": a.rounds, "calls_per_round": a.calls, "reference": "append_tokens n=1 + attend_tokens Nq=1 on a contiguous cache",
           "candidates": {f"paged{pr}": f"append_paged n=1 + attend_paged Nq=1, {pr} rows a page, randomly permuted table"
                          for pr in PAGE_SIZES},
           "bit_identical_to_contiguous": same, "reference_is_finite_and_nonzero": sane}
    for i, what in enumerate(names):
        res[f"ref_{what}_ms"] = round(med["contiguous"][i], 5)
        res[f"ref_{what}_spread"] = round(spread[i], 4)
        for pr in PAGE_SIZES:
            res[f"paged{pr}_{what}_ms"] = round(med[f"paged{pr}"][i], 5)
            res[f"paged{pr}_{what}_ratio"] = round(med[f"paged{pr}"][i] / med["contiguous"][i], 4)
    res.update({"per_round": {s: [[round(x, 5) for x in row] for row in per[s]] for s in per},
                "memory": memory,
                "not_measured": ["prefill through pages", "other head sizes", "grouped caches", "a captured step against an eager one"],
                "clock_probe": bench.clock_probe(dev),
                "isa_sha16": {"ragged_main": isa_id.isa_sha16(_lib.LIB_PATH, f"qmha_fa_{stem}_cache_kernelILi{a.d}ENS_6RaggedEEEv"),
                              "paged_main": isa_id.isa_sha16(_lib.LIB_PATH, f"qmha_fa_{stem}_cache_kernelILi{a.d}ENS_5PagedEEEv"),
                              "token_append": isa_id.isa_sha16(_lib.LIB_PATH, f"qmha_kv_rows_{stem}_kernelILi{a.d}ENS_11UniformRowsENS_14ContiguousRowsE"),
                              "paged_append": isa_id.isa_sha16(_lib.LIB_PATH, f"qmha_kv_rows_{stem}_kernelILi{a.d}ENS_11UniformRowsENS_10PagedTableE")},
                "device": torch.cuda.get_device_properties(dev).name})
    print(json.dumps(res), flush=True)
    if not (all(same.values()) and sane):
        sys.exit("paged_ab: a paged O is not the contiguous cache's")


if __name__ == "__main__":
    main()
