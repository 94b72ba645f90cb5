"""What the packed-batch tests share: a Python restatement of the index arithmetic of the packed kernels,
and the yardstick builders that define what a packed call must return.

The restatement follows the kernels line by line -- tests/test_packed_cpu.py ties its formulas to the source with
verbatim line checks -- and never touches a GPU:
  * packed_seq / ragged_geo: the attend prologue (qmha_fa_masked.hpp's packed_seq, Ragged::of): the validity rules, nq_b,
    s, Nq', Ga, GL, diag_off, and the memory row of a lane;
  * packed_item / item_groups: the append's items (qmha_prepass.hip's packed_item, token_groups_*): g0, g1, the source
    row, and maxg from max_n.

The yardstick builders run what shipped before the packed calls: for every distinct count c of a packed call, the
existing attend_tokens / append_tokens (or the paged ones) with Nq = c / n = c on a padded [B, c, ...] buffer, every
sequence of another count switched off through an invalid lens / pos entry; the rows (or the cache bytes) of the
sequences that have count c are what the packed call must give, bit for bit.  They take the call as a function, so the
same builder serves a contiguous cache, a paged one and either binding.
"""
GROUP, WAVES = 32, 4
SKIP, ZERO, RUN = "skip", "zero", "run"  # nothing read or written / the range's rows of O zeroed / the body runs


def ceil32(x):
    return (x + GROUP - 1) & ~(GROUP - 1)


# ---- the attend prologue ---------------------------------------------------------------------------------------------------
def max_units(max_nq, G=1):
    """Ragged::max_units at Nq = max_nq: the units the grid is sized for."""
    return G * ((max_nq + 2 * GROUP - 2) // GROUP)


def nqb_of(units):
    """masked_nqb: unit blocks of a K/V slice."""
    return (units + WAVES - 1) // WAVES


def ragged_geo(nq, L):
    """Ragged::of(L) at Nq = nq: s, Nq', GL, Ga, diag_off."""
    s = (L - nq) & (GROUP - 1)
    Lp, Nqp = ceil32(L), ceil32(s + nq)
    return {"nq": nq, "s": s, "Nqp": Nqp, "GL": Lp // GROUP, "Ga": Nqp // GROUP, "diag_off": (Lp - Nqp) // GROUP}


def packed_seq(c0, c1, total, max_nq, L, cap, pages_ok=True):
    """packed_seq of qmha_fa_masked.hpp for a sequence with cu[b] = c0, cu[b + 1] = c1: (verdict, row0, nq_b).  L is looked
    at only when the range is in bounds, not empty and within max_nq; pages_ok: the paged kernels' table scan."""
    if c0 < 0 or c1 < c0 or c1 > total:
        return SKIP, 0, 0
    if c1 == c0:
        return SKIP, 0, 0
    row0, nq = c0, c1 - c0
    if nq > max_nq:
        return ZERO, row0, nq
    if L < nq or L > cap:
        return ZERO, row0, nq
    if not pages_ok:
        return ZERO, row0, nq
    return RUN, row0, nq


def lane_row(row0, geo, qg, col):
    """The memory row of lane `col` of query group qg (int8: 32 qg + col; fp16: 32 qg + 16 qb + r16, the same set), or
    None for a pad lane: row_real / row_shift over seq_row0."""
    r = GROUP * qg + col - geo["s"]
    return row0 + r if 0 <= r < geo["nq"] else None


def last_tile(geo, qg):
    """Varlen::last: the last key tile query group qg visits."""
    return min(qg + geo["diag_off"], geo["GL"] - 1)


# ---- the append's items ------------------------------------------------------------------------------------------------------
def token_items(n):
    """Items of a K/V slice for n rows: a wave per touched group, the first wave taking the last group too."""
    return 1 if n <= 2 else (n + GROUP - 2) // GROUP


def packed_item(c0, c1, rows, max_n, p, cap, j):
    """packed_item of qmha_prepass.hip for item j of a sequence: None (the wave returns) or (n_b, row0, g0, g1, groups the
    item runs)."""
    if c0 < 0 or c1 < c0 or c1 > rows:
        return None
    n = c1 - c0
    if n == 0 or n > max_n:
        return None
    if p < 0 or p > cap - n:
        return None
    g0, g1 = p // GROUP, (p + n - 1) // GROUP
    if not (j == 0 or j < g1 - g0):
        return None
    groups = [g0 + j] + ([g1] if j == 0 and g1 != g0 else [])  # item 0: g0 and then g1, reading the tail before it writes it
    return n, c0, g0, g1, groups


def group_rows(p, n, row0, g):
    """token_groups_*: for group g, {row of the group: source row in K / V} of the new rows, the rows of the group that come
    from the tail (ahead of p, group g0 only), and whether the group stays open (its new rows go to the tail)."""
    lo, hi = p - g * GROUP, p - g * GROUP + n
    new = {r: row0 + (r - lo) for r in range(GROUP) if lo <= r < hi}
    tail = [r for r in range(GROUP) if r < lo and r < hi]
    stays_open = g == (p + n - 1) // GROUP and (p + n) % GROUP != 0
    return new, tail, stays_open


# ---- the yardstick builders -----------------------------------------------------------------------------------------------
def counts_of(cu):
    return [cu[b + 1] - cu[b] for b in range(len(cu) - 1)]


def yard_attend(attend, Qp, cu, lens, skip=()):
    """{b: numpy [count_b, d_model]} for every sequence with a count above 0 that is not in `skip`: per distinct count c,
    attend(Qpad [B, c, d_model], lens') -- attend_tokens or attend_paged, returning numpy [B, c, d_model] -- where lens' is
    lens[b] for the sequences of count c and 0 (invalid: below Nq) for the others.  cu: a monotone host list."""
    import torch
    counts, want = counts_of(cu), {}
    for c in sorted(set(counts) - {0}):
        mine = [b for b, n in enumerate(counts) if n == c and b not in skip]
        if not mine:
            continue
        Qpad = torch.zeros((len(counts), c, Qp.shape[1]), dtype=torch.float32, device=Qp.device)
        for b in mine:
            Qpad[b] = Qp[cu[b]:cu[b + 1]]
        out = attend(Qpad, [lens[b] if b in mine else 0 for b in range(len(counts))])
        for b in mine:
            want[b] = out[b]
    return want


def yard_append(append, Kp, Vp, cu, pos, skip=()):
    """Per distinct count c, append(Kpad, Vpad [B, c, width], pos') -- append_tokens or append_paged -- where pos' is pos[b] for
    the sequences of count c that are not in `skip` and -1 (invalid) for the others.  cu: a monotone host list."""
    import torch
    counts = counts_of(cu)
    for c in sorted(set(counts) - {0}):
        mine = [b for b, n in enumerate(counts) if n == c and b not in skip]
        if not mine:
            continue
        Kpad, Vpad = (torch.zeros((len(counts), c, Kp.shape[1]), dtype=torch.float32, device=Kp.device) for _ in range(2))
        for b in mine:
            Kpad[b], Vpad[b] = Kp[cu[b]:cu[b + 1]], Vp[cu[b]:cu[b + 1]]
        append(Kpad, Vpad, [pos[b] if b in mine else -1 for b in range(len(counts))])
