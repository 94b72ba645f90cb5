#!/usr/bin/env python3
"""A serving step through the packed calls (qmha_kv_cache_append_packed plus qmha_attend_cached_packed)
against the step the library offered before, in one process, alternating.

    python tools/packed_ab.py --mode decode --variant fa_tc_int8_b --B 16 --H 16 --d 64 --cap 4096
    python tools/packed_ab.py --mode mixed  --variant fa_tc_v1a

Two caches of `cap` rows are filled once, one for each side.  Sequence b holds L[b] = 32 t[b] + 17 rows, t[b] spread evenly
over 512 / 32 .. cap / 32 - 1, its open group built by append_tokens from its first row on.
  decode  every sequence brings one row.  Candidate: append_packed + attend_packed with every count 1.  Reference:
          append_tokens n = 1 + attend_tokens Nq = 1.  The tile counts are equal, so the main-kernel ratio is expected at 1.
  mixed   two sequences (--prefill rows each, at a multiple of 32) are in chunked prefill, the others decode one row.
          Candidate: ONE append_packed + attend_packed at max_n = max_nq = --prefill.  Reference: the two launch pairs the
          library needed before -- append_tokens + attend_tokens at Nq = --prefill with the decoding sequences switched off
          (pos = -1, lens = 0), then at Nq = 1 with the prefilling ones switched off --, over padded [B, Nq, d_model] buffers.
          The reference's main-kernel figure is the sum of its two main kernels.
With qmha_profile on, both sides are warmed, then ROUNDS rounds alternate CALLS reference and CALLS candidate steps; the
figures are the library's own event pairs (append: pre-pass, attend: main kernel) and a device-event pair around each
batch (the whole step, launches included).  Medians over the rounds; spread = (max - min) / median of the reference's own
rounds.  One JSON line.  Before anything is timed the candidate's O is compared bit for bit with the reference's rows.
--control: an A/A run -- the candidate side runs the reference's own calls on the candidate's cache --, which shows what
the two caches' placement alone is worth, the floor under any ratio this tool reports.
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
    ap.add_argument("--mode", default="decode", choices=["decode", "mixed"])
    ap.add_argument("--variant", default="fa_tc_int8_b", choices=["fa_tc_int8_b", "fa_tc_v1a"])
    ap.add_argument("--B", type=int, default=16)
    ap.add_argument("--H", type=int, default=16)
    ap.add_argument("--d", type=int, default=64)
    ap.add_argument("--cap", type=int, default=4096)
    ap.add_argument("--prefill", type=int, default=512)
    ap.add_argument("--control", action="store_true",
                    help="A/A: the candidate side runs the reference's calls on the candidate's cache (what two caches alone differ by)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    if a.rounds < 5 or a.calls < 30:
        ap.error("at least 5 rounds of at least 30 calls")
    if a.cap % 32 or a.cap < 1024 or a.B < 4 or a.prefill % 32 or not 32 <= a.prefill <= 512:
        ap.error("cap % 32 == 0, cap >= 1024, B >= 4, prefill a multiple of 32 in [32, 512]")

    import torch
    import bench
    from quantizedmha_amd import _lib, isa_id, torch_ext
    lib = _lib.load()
    dev = torch.device("cuda:0")
    dm, r, P = a.H * a.d, 17, a.prefill
    g = torch.Generator(device=dev).manual_seed(a.cap + a.d)
    K, V = (torch.rand((a.B, a.cap, dm), generator=g, device=dev, dtype=torch.float32) for _ in range(2))
    Q = torch.rand((a.B, P, dm), generator=g, device=dev, dtype=torch.float32)
    stream = torch.cuda.current_stream(dev).cuda_stream
    stem = "int8" if a.variant == "fa_tc_int8_b" else "f16"
    CAUSAL = _lib.QMHA_FLAG_CAUSAL
    i32 = lambda xs: torch.tensor(xs, dtype=torch.int32, device=dev)  # noqa: E731

    t0, t1 = 512 // 32, a.cap // 32 - 1
    tiles = [t0 + round(i * (t1 - t0) / (a.B - 1)) for i in range(a.B)]
    pre = [a.B // 3, 2 * a.B // 3] if a.mode == "mixed" else []  # the sequences in chunked prefill
    L = [32 * t if b in pre else 32 * t + r for b, t in enumerate(tiles)]  # rows held after the step
    counts = [P if b in pre else 1 for b in range(a.B)]
    pos = [L[b] - counts[b] for b in range(a.B)]
    cu = [0]
    for n in counts:
        cu.append(cu[-1] + n)
    total = cu[-1]
    rows = lambda X, first, n: torch.stack([X[b, p:p + n] for b, p in enumerate(first)]).contiguous()  # noqa: E731

    cand, ref = (torch_ext.KVCache(a.B, a.cap, dm, a.H, a.variant, device=dev) for _ in range(2))
    base = [32 * t for t in tiles]
    for c in (cand, ref):
        c.append(K, V)
        c.enable_tokens()
        # the decoding sequences' open group, from its first row on (the prefilling ones are left out)
        c.append_tokens(rows(K, base, r - 1), rows(V, base, r - 1), i32([-1 if b in pre else base[b] for b in range(a.B)]))

    # the candidate's operands: no batch axis
    kp = torch.cat([K[b, pos[b]:L[b]] for b in range(a.B)]).contiguous()
    vp = torch.cat([V[b, pos[b]:L[b]] for b in range(a.B)]).contiguous()
    qp = torch.cat([Q[b, :counts[b]] for b in range(a.B)]).contiguous()
    op = torch.empty_like(qp)
    cu_d, pos_d, lens_d = i32(cu), i32(pos), i32(L)
    bound = max(counts)

    def packed_step():
        _lib.check(lib.qmha_kv_cache_append_packed(cand._handle, kp.data_ptr(), vp.data_ptr(), total, bound, cu_d.data_ptr(),
                                                   pos_d.data_ptr(), stream), "append_packed")
        _lib.check(lib.qmha_attend_cached_packed(cand._handle, qp.data_ptr(), op.data_ptr(), total, bound, cu_d.data_ptr(),
                                                 lens_d.data_ptr(), CAUSAL, stream), "attend_packed")

    # the reference's operands: one padded [B, n, d_model] set per distinct count, the other sequences switched off
    groups = []
    for n in sorted(set(counts), reverse=True):
        mine = [b for b in range(a.B) if counts[b] == n]
        first = [pos[b] if b in mine else 0 for b in range(a.B)]
        groups.append((n, mine, rows(K, first, n), rows(V, first, n), Q[:, :n].contiguous(), torch.empty((a.B, n, dm), device=dev),
                       i32([pos[b] if b in mine else -1 for b in range(a.B)]), i32([L[b] if b in mine else 0 for b in range(a.B)])))

    def tokens_step(cache=ref):
        for n, _, k, v, q, o, p_d, l_d in groups:
            _lib.check(lib.qmha_kv_cache_append_tokens(cache._handle, k.data_ptr(), v.data_ptr(), n, p_d.data_ptr(), stream), "append_tokens")
            _lib.check(lib.qmha_attend_cached_tokens(cache._handle, q.data_ptr(), o.data_ptr(), n, l_d.data_ptr(), CAUSAL, stream),
                       "attend_tokens")

    # O before timing: the candidate's rows against the reference's
    packed_step()
    tokens_step()
    torch.cuda.synchronize(dev)
    same = bool(torch.isfinite(op).all()) and float(op.abs().max()) > 0.0
    for n, mine, _, _, _, o, _, _ in groups:
        for b in mine:
            same = same and bool(torch.equal(op[cu[b]:cu[b + 1]], o[b]))
    same = same and bool(torch.equal(cand.mem, ref.mem)) and bool(torch.equal(cand.tail, ref.tail))

    def batch(call, n, records):
        """n steps: (main-kernel ms, pre-pass ms, whole-step ms) per step."""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            call()
        e1.record()
        torch.cuda.synchronize(dev)
        main_ms, pre_ms, k = ctypes.c_double(), ctypes.c_double(), ctypes.c_longlong()
        _lib.check(lib.qmha_profile_collect(ctypes.byref(main_ms), ctypes.byref(k), ctypes.byref(pre_ms)), "collect")
        assert k.value == records * n, (k.value, records, n)  # one record per append, one per attend
        return main_ms.value / n, pre_ms.value / n, e0.elapsed_time(e1) / n

    sides = {"tokens": (tokens_step, 2 * len(groups)), "packed": (packed_step, 2)}  # the reference first
    if a.control:
        sides["packed"] = (lambda: tokens_step(cand), 2 * len(groups))
    lib.qmha_profile_collect(None, None, None)
    lib.qmha_profile_enable(1)
    try:
        for call, rec in sides.values():
            batch(call, a.warmup, rec)
        per = {s: [] for s in sides}
        for _ in range(a.rounds):
            for s, (call, rec) in sides.items():
                per[s].append(batch(call, a.calls, rec))
    finally:
        lib.qmha_profile_enable(0)
    med = {s: [statistics.median(x[i] for x in per[s]) for i in range(3)] for s in per}
    spread = lambda i: round((max(x[i] for x in per["tokens"]) - min(x[i] for x in per["tokens"])) / med["tokens"][i], 4)  # noqa: E731
    res = {"tool": "packed_ab", "mode": a.mode, "control": a.control, "variant": a.variant, "B": a.B, "H": a.H, "d": a.d, "cap": a.cap, "lens": L,
           "counts": counts, "total": total, "bound": bound, "rounds": a.rounds, "calls_per_round": a.calls,
           "reference": " then ".join(f"append_tokens n={n} + attend_tokens Nq={n}" for n, *_ in groups),
           "candidate": f"append_packed + attend_packed, max_n = max_nq = {bound}", "bit_identical_to_reference": same,
           "ref_main_kernel_ms": round(med["tokens"][0], 5), "packed_main_kernel_ms": round(med["packed"][0], 5),
           "ref_append_ms": round(med["tokens"][1], 5), "packed_append_ms": round(med["packed"][1], 5),
           "ref_step_ms": round(med["tokens"][2], 5), "packed_step_ms": round(med["packed"][2], 5),
           "main_ratio": round(med["packed"][0] / med["tokens"][0], 4), "ref_main_spread": spread(0),
           "append_ratio": round(med["packed"][1] / med["tokens"][1], 4), "ref_append_spread": spread(1),
           "step_ratio": round(med["packed"][2] / med["tokens"][2], 4), "ref_step_spread": spread(2),
           "per_round": {s: [[round(x, 5) for x in row] for row in per[s]] for s in per},
           "clock_probe": bench.clock_probe(dev),
           "isa_sha16": {"ragged_main": isa_id.isa_sha16(_lib.LIB_PATH, f"qmha_fa_{stem}_cache_kernelILi{a.d}ENS_6RaggedEEEv"),
                         "packed_main": isa_id.isa_sha16(_lib.LIB_PATH, f"qmha_fa_{stem}_cache_kernelILi{a.d}ENS_6PackedINS_6RaggedEEEEEv")},
           "device": torch.cuda.get_device_properties(dev).name}
    print(json.dumps(res), flush=True)
    if not same:
        sys.exit("packed_ab: the candidate's O or cache is not the reference's")


if __name__ == "__main__":
    main()
