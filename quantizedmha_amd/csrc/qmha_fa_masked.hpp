// qmha_fa_masked.hpp -- what the translation units of the masked kernel bodies share (qmha_fa_masked.hip,
// qmha_fa_split.hip, qmha_fa_packed.hip, qmha_fa_window.hip; the modes are described at the top of the first): the geometries of a launch,
// the launch-index maps, the K/V stager, the zeroing helpers, the attend kernels of a persistent K/V cache
// (qmha_fa_{int8,f16}_cache_kernel) and the checked geometry of a call (masked_geo).  The three files stay three
// translation units: the dumping twins of qmha_fa_masked.hip reach their out-of-line dump lambdas PC-relative, so a
// kernel added to their code object shows in their bytes.
#pragma once

#include "qmha_common.hpp"
#include "qmha_kernels.hpp"

#include <type_traits>

namespace qmha {

static constexpr float kLazySumCapC = 4096.0f;  // the fp16 lazy base's cap
constexpr int kWaves = 4, kSG = 2;

// The geometry of a launch, a kernel argument: the rows of Q / O and of K / V, and which key tiles query
// group g visits -- tiles t <= last(g), masked on tile diag(g).  And the units of a K/V slice (the header's
// "Units"): how many, and which query group and query head unit u is.
// Square causal: the diagonal of group g is tile g, which is also its last; nothing beyond N is passed or
// computed, so these instances carry no offset and no clamp.
struct SquareCausal {
    static constexpr bool kDump = false;
    int N;
    __device__ int nq() const { return N; }
    __device__ int nk() const { return N; }
    __device__ int gk() const { return N / QMHA_GROUP; }
    __device__ int diag(int g) const { return g; }
    __device__ int last(int g) const { return g; }
    __host__ __device__ int units() const { return N / QMHA_GROUP; }
    __device__ int group(int u) const { return u; }
    __device__ int head(int kvh, int u) const { return kvh; }
};
// Rectangular.  causal: bottom-right aligned, diag_off = Gk - Gq (Nk >= Nq, checked by the launchers);
// else diag_off = Gk, a diagonal no tile reaches
struct Rect {
    static constexpr bool kDump = false;
    int Nq, Nk, diag_off;
    Rect(int nq, int nk, bool causal) : Nq(nq), Nk(nk), diag_off(nk / QMHA_GROUP - (causal ? nq / QMHA_GROUP : 0)) {}
    // Host only: the causal geometry of a K/V cache.  The arrays hold `cap` rows per head slice and the
    // first `len` are valid: Nk = cap keeps the bases, the extents and the sK / sV index those of the cache, and the
    // explicit offset (len - nq) / 32 puts the diagonal of the last query group on tile len / 32 - 1, so last(g) <=
    // len / 32 - 1 for every g < Gq and no tile at or beyond len / 32 is staged or computed.  nq <= len <= cap.
    static Rect cached(int nq, int cap, int len) {
        Rect r(nq, cap, false);
        r.diag_off = (len - nq) / QMHA_GROUP;
        return r;
    }
    __device__ int nq() const { return Nq; }
    __device__ int nk() const { return Nk; }
    __device__ int gk() const { return Nk / QMHA_GROUP; }
    __device__ int diag(int g) const { return g + diag_off; }  // >= Gk: none
    __device__ int last(int g) const { return min(g + diag_off, gk() - 1); }
    __host__ __device__ int units() const { return Nq / QMHA_GROUP; }
    __device__ int group(int u) const { return u; }
    __device__ int head(int kvh, int u) const { return kvh; }
};
// Grouped-query: Rect's rows and diagonal (its cached form too), and G query heads per K/V head.  The divisions
// are unsigned: scalar, through a reciprocal, as the launch-index ones are.
struct Grouped : Rect {
    int G;
    Grouped(Rect r, int g) : Rect(r), G(g) {}
    __host__ __device__ int units() const { return G * (Nq / QMHA_GROUP); }
    __device__ int group(int u) const { return (int)((unsigned)u / (unsigned)G); }
    __device__ int head(int kvh, int u) const { return kvh * G + (int)((unsigned)u % (unsigned)G); }
};

// Per-sequence lengths read on the device: Grouped's units over a cache of Nk = cap rows (G = 1: a
// multi-head cache, where Grouped's unit map is Rect's), of which sequence b attends its first L = lens[b].  The host
// fills Nq, Nk, G and the mode; the kernel loads L and forms that sequence's geometry with of(L) before the body
// sees it: diag_off = (L - Nq) / 32 (causal, Rect::cached at len = L) or Gk (no diagonal), and GL = L / 32 tiles, which
// clamps last(g) where Rect clamps at Gk.  Nk = cap keeps the bases, the extents and the sK / sV index, so whatever
// L is, a valid sequence issues whole tiles t <= GL - 1 <= Gk - 1 only.
struct Varlen : Grouped {
    int GL;  // tiles of this sequence
    bool causal;
    Varlen(int nq, int cap, int g, bool c) : Grouped(Rect(nq, cap, false), g), GL(0), causal(c) {}
    // L % 32 == 0 (two's complement: also of a negative L, which the lower bound rejects), L <= cap, and Nq rows
    // (causal, bottom-right aligned) or one tile (no mask) to attend
    __device__ bool valid(int L) const { return (L & (QMHA_GROUP - 1)) == 0 && L <= Nk && L >= (causal ? Nq : QMHA_GROUP); }
    __device__ Varlen of(int L) const {
        Varlen v = *this;
        v.GL = L / QMHA_GROUP;
        v.diag_off = causal ? (L - Nq) / QMHA_GROUP : gk();
        return v;
    }
    __device__ int last(int g) const { return min(g + diag_off, GL - 1); }
};

// Token-granular lengths: Nq query rows (any 1 <= Nq <= cap) attend the first L = lens[b] rows of a
// causal cache, bottom-right aligned, for any Nq <= L <= cap.  Absolute row positions keep their 32-row groups: with
// s = (L - Nq) mod 32 the call is Varlen's causal one on a zero [Nq', d_model] block, Nq' = ceil32(s + Nq), that holds Q
// at rows [s, s + Nq), against L' = ceil32(L) rows -- L' - Nq' = L - Nq - s is a multiple of 32, so the diagonal tile
// and its in-tile mask are the existing ones, and the mask hides exactly the key rows >= L from every real query row.
// Nq stays the caller's row count (the batch stride of Q and O); the padded block exists in registers only: a lane
// whose memory row 32 qg + col - s lies outside [0, Nq) holds zeros without a load and stores nothing (row_real,
// row_shift below).  The grid cannot follow s: the host sizes it for ceil((Nq + 31) / 32) query groups per head
// (max_units), of which a sequence has Ga = Nq' / 32 active -- the body's U --, and a workgroup with no active unit
// leaves before its first barrier.
struct Ragged : Varlen {
    int s;   // rows of padding ahead of Q in its first group
    int Ga;  // active query groups of this sequence
    Ragged(int nq, int cap, int g) : Varlen(nq, cap, g, true), s(0), Ga(0) {}
    __host__ __device__ int max_units() const { return G * ((Nq + 2 * QMHA_GROUP - 2) / QMHA_GROUP); }
    __device__ bool valid(int L) const { return L >= Nq && L <= Nk; }
    __device__ Ragged of(int L) const {
        Ragged v = *this;
        v.s = (L - Nq) & (QMHA_GROUP - 1);
        const int Lp = (L + QMHA_GROUP - 1) & ~(QMHA_GROUP - 1), Nqp = (v.s + Nq + QMHA_GROUP - 1) & ~(QMHA_GROUP - 1);
        v.GL = Lp / QMHA_GROUP;  // <= Gk: cap is a multiple of 32
        v.Ga = Nqp / QMHA_GROUP;
        v.diag_off = (Lp - Nqp) / QMHA_GROUP;
        return v;
    }
    __host__ __device__ int units() const { return G * Ga; }
};
// A paged cache: Ragged's rows, queries and diagonal over a logical capacity Nk = max_pages * page_rows
// whose rows lie in pages of a pool.  Row r of sequence b is row r % page_rows of page table[b][r / page_rows]; page p,
// K/V head kvh is slice p * H + kvh of a carve at (num_pages, page_rows, H), so a page slice has the layout of a
// contiguous slice of page_rows rows and the tile arithmetic does not change.  page_rows % 64 == 0: a stage of kSG = 2
// tiles lies in one page.  The table is read on the device: the used entries are checked by every wave before the
// workgroup's first barrier or DMA issue (used_pages_ok), and the entry a stage is issued with (entry) is clamped
// into the pool, so no table content can become an address outside it.
struct Paged : Ragged {
    const int32_t* table;  // DEVICE int32 [B][max_pages]
    int PG;                // 32-row groups of a page (even)
    int max_pages, num_pages;
    Paged(Ragged r, const int32_t* t, int page_rows, int mp, int np) : Ragged(r), table(t), PG(page_rows / QMHA_GROUP), max_pages(mp), num_pages(np) {}
    __device__ Paged of(int L) const {
        Paged v = *this;
        static_cast<Ragged&>(v) = Ragged::of(L);
        return v;
    }
    // every entry of the pages that the first L rows of sequence b use lies in [0, num_pages): lanes take the columns,
    // a ballot joins them -- the same verdict in every wave.  Columns behind the used pages are not loaded.
    __device__ bool used_pages_ok(int b, int L) const {
        const int lane = threadIdx.x & 63;
        bool bad = false;
        for (int c = lane; c < max_pages; c += 64)
            if (c * (PG * QMHA_GROUP) < L) bad |= (unsigned)table[(size_t)b * max_pages + c] >= (unsigned)num_pages;
        return __builtin_amdgcn_ballot_w64(bad) == 0;
    }
    // the windowed form: the pages that hold rows [lo, L) of sequence b, lo a stage's first row.  Columns
    // wholly behind row lo are not loaded either.
    __device__ bool used_pages_ok(int b, int lo, int L) const {
        const int lane = threadIdx.x & 63;
        bool bad = false;
        for (int c = lane; c < max_pages; c += 64)
            if (c * (PG * QMHA_GROUP) < L && (c + 1) * (PG * QMHA_GROUP) > lo) bad |= (unsigned)table[(size_t)b * max_pages + c] >= (unsigned)num_pages;
        return __builtin_amdgcn_ballot_w64(bad) == 0;
    }
    // column c of sequence b's table row, wave-uniform; the column and the id are clamped to the row and the pool.  Read
    // through the constant address space -- no kernel writes a table --, which makes it a scalar load: a vector load
    // would be waited for with vmcnt(0), together with the stage's DMA that was just issued.
    __device__ int entry(int b, int c) const {
        typedef const int32_t __attribute__((address_space(4))) * ConstI32;
        const int e = *(ConstI32)(uintptr_t)(table + (size_t)b * max_pages + min(c, max_pages - 1));
        return (int)min((unsigned)e, (unsigned)(num_pages - 1));
    }
};
// The pages of a workgroup's stages in issue order (stage 0, 1, ... of a pass).  take(): page / tile0 / sip become those
// of the stage about to be issued -- which is the stage computed next, so the id a stage computes with (sK / sV) is the
// id it was issued with.  advance(), behind the DMA issue: `next`, the entry of the stage to issue after that, is loaded
// a stage ahead of its use, so the scalar load does not stand in front of a DMA issue.
struct PageWalk {
    int col, sip_next, next;  // the next stage to issue: table column, stage within its page, entry
    int page, tile0, sip;     // the stage issued last: page id, first tile of its page, stage within its page
    __device__ __forceinline__ void start(const Paged& g, int b) {
        col = 0, sip_next = 0;
        next = g.entry(b, 0);
    }
    // a pass that begins at tile t0 (even: a stage's first): a chunk of a split sweep
    __device__ __forceinline__ void start_at(const Paged& g, int b, int t0) {
        col = t0 / g.PG, sip_next = t0 % g.PG / kSG;
        next = g.entry(b, col);
    }
    __device__ __forceinline__ void take(const Paged& g) { page = next, tile0 = col * g.PG, sip = sip_next; }
    __device__ __forceinline__ void advance(const Paged& g, int b) {
        if (++sip_next == g.PG / kSG) {
            sip_next = 0;
            next = g.entry(b, ++col);
        }
    }
};
struct NoWalk {};

// Split-KV: Ragged's or Paged's call with the key sweep cut into chunks of C tiles (C even: a chunk is a
// whole number of stages, and in a pool never cuts a page's stage).  A workgroup is one unit block of one chunk c < NC
// (c from the launch index): its waves run tiles c C ... min(c C + C - 1, last(qg)) from the zero state and
// store the epilogue's O, l and m of those tiles alone into the caller's scratch (SplitScratch, qmha_kernels.hpp); a
// wave whose last(qg) lies before c C takes no part in the arithmetic and stores nothing.  qmha_split_combine_kernel
// joins the chunks.  first() / end(): the chunk's first tile and its last.
template <class Geo>
struct Split : Geo {
    float *Oc, *pm, *pl;  // [B][NC][Nq][h D], [B][NC][Nq][h], [B][NC][Nq][h]
    int C, NC;            // tiles per chunk, chunks
    int c;                // device: the workgroup's chunk
    Split(Geo g, const SplitScratch& s, int tiles, int chunks) : Geo(g), Oc(s.Oc), pm(s.m), pl(s.l), C(tiles), NC(chunks), c(0) {}
    __device__ Split of(int L, int chunk) const {
        Split v = *this;
        static_cast<Geo&>(v) = Geo::of(L);
        v.c = chunk;
        return v;
    }
    __device__ int first() const { return c * C; }
    __device__ int end() const { return c * C + C - 1; }
};
template <class T>
struct IsSplit : std::false_type {};
template <class Geo>
struct IsSplit<Split<Geo>> : std::true_type {};

// Packed batches: Ragged's or Paged's call on operands without a batch axis.  Q and O are
// [total, d_model]; sequence b owns the rows [cu[b], cu[b + 1]) (cu: DEVICE int32 [B + 1]), so it brings a query count
// of its own, nq_b = cu[b + 1] - cu[b].  The host's Nq is the bound max_nq the grid is sized for (Ragged::max_units);
// the kernel's prologue (packed_seq below) checks the range, nq_b and lens[b] and then forms the sequence's geometry
// with of(): Base's geometry at Nq = nq_b -- what the unpacked call forms for a batch of that Nq --, and row0 = cu[b],
// the first row of the sequence in Q and O, where the other geometries have b * Nq (seq_row0 below).
template <class Base>
struct Packed : Base {
    const int32_t* cu;  // DEVICE int32 [B + 1]
    int total;          // rows of Q and O
    int row0;           // device: the sequence's first row
    Packed(Base g, const int32_t* c, int t) : Base(g), cu(c), total(t), row0(0) {}
    __device__ Packed of(int first, int nq, int L) const {
        Packed v = *this;
        v.Nq = nq;
        static_cast<Base&>(v) = static_cast<const Base&>(v).of(L);
        v.row0 = first;
        return v;
    }
};
template <class T>
struct IsPacked : std::false_type {};
template <class Base>
struct IsPacked<Packed<Base>> : std::true_type {};

// A sliding window: Ragged's or Paged's call in which a query row sees only the last `window` = 32 w keys of
// those the causal mask leaves it (w >= 1).  Absolute row positions keep their 32-row groups, so the window's left edge of
// query group qg falls in tile left(qg) = diag(qg) - w with the complement of the diagonal's in-tile mask (key column c is
// visible to row r iff c > r), the tiles strictly between the two are unmasked, and the sweep of the group is tiles
// first(qg) = max(0, left(qg)) ... diag(qg) from the zero state.  left(qg) < 0: no left tile.  A workgroup is one unit
// block (no pair: a band has no triangle to balance); t0, set by of() for unit block qb, is the first tile of its first
// stage -- first() is monotone in the unit, so that of the block's first unit, rounded down to a stage.
template <class Base>
struct Window : Base {
    int w;   // tiles of the window
    int t0;  // device: the first tile of the workgroup's first stage (even)
    Window(Base g, int tiles) : Base(g), w(tiles), t0(0) {}
    __device__ int left(int qg) const { return this->diag(qg) - w; }
    __device__ int first(int qg) const { return max(left(qg), 0); }
    __device__ Window of(int L, int qb) const {
        Window v = *this;
        static_cast<Base&>(v) = Base::of(L);
        v.t0 = v.first(v.group(qb * kWaves)) & ~(kSG - 1);
        return v;
    }
};
template <class T>
struct IsWindow : std::false_type {};
template <class Base>
struct IsWindow<Window<Base>> : std::true_type {};

// A lane's row of Q / O in memory is its row of the (padded) block less row_shift; row_real: that row exists.
// Constants for every geometry but Ragged (and Paged over it), so the other instances carry no trace of them.
template <class Geo>
constexpr bool kRaggedGeo = std::is_base_of<Ragged, std::remove_cv_t<Geo>>::value;
template <class Geo>
constexpr bool kPagedGeo = std::is_base_of<Paged, std::remove_cv_t<Geo>>::value;
template <class Geo>
constexpr bool kSplitGeo = IsSplit<std::remove_cv_t<Geo>>::value;
// a value of a type that depends on D: the bodies' `if constexpr` branches over a geometry are discarded unchecked
template <int D, class T>
__device__ __forceinline__ T as_dependent(T t) { return t; }
template <class Geo>
__device__ __forceinline__ constexpr int row_shift(const Geo&) { return 0; }
template <class Geo>
__device__ __forceinline__ constexpr bool row_real(const Geo&, int) { return true; }
__device__ __forceinline__ int row_shift(const Ragged& g) { return g.s; }
__device__ __forceinline__ bool row_real(const Ragged& g, int row) { return (unsigned)(row - g.s) < (unsigned)g.Nq; }
__device__ __forceinline__ int row_shift(const Paged& g) { return g.s; }
__device__ __forceinline__ bool row_real(const Paged& g, int row) { return (unsigned)(row - g.s) < (unsigned)g.Nq; }
template <class Geo>
__device__ __forceinline__ int row_shift(const Split<Geo>& g) { return g.s; }
template <class Geo>
__device__ __forceinline__ bool row_real(const Split<Geo>& g, int row) { return (unsigned)(row - g.s) < (unsigned)g.Nq; }
template <class Geo>
__device__ __forceinline__ int row_shift(const Packed<Geo>& g) { return g.s; }
template <class Geo>
__device__ __forceinline__ bool row_real(const Packed<Geo>& g, int row) { return (unsigned)(row - g.s) < (unsigned)g.Nq; }
template <class Geo>
__device__ __forceinline__ int row_shift(const Window<Geo>& g) { return g.s; }
template <class Geo>
__device__ __forceinline__ bool row_real(const Window<Geo>& g, int row) { return (unsigned)(row - g.s) < (unsigned)g.Nq; }
template <class Geo>
constexpr bool kWindowGeo = IsWindow<std::remove_cv_t<Geo>>::value;
// The first row of a sequence in Q and O: slice * Nq where the operands have a batch axis (slice: b, or Split's
// (b, chunk) slice of the scratch); a packed sequence's cu[b].  kPackedGeo: the int8 body takes the second under
// `if constexpr`, as it takes row_shift and row_real.
template <class Geo>
constexpr bool kPackedGeo = IsPacked<std::remove_cv_t<Geo>>::value;
template <class Geo>
__device__ __forceinline__ size_t seq_row0(const Geo& g, int slice) { return (size_t)slice * g.nq(); }
template <class Geo>
__device__ __forceinline__ size_t seq_row0(const Packed<Geo>& g, int) { return (size_t)g.row0; }
// The tiles a workgroup may visit and where its stores go: every tile and O itself, but for Split its chunk and the
// scratch's Oc, whose slice (b, c) has the layout of O's slice b.  Constants for every other geometry.
template <class Geo>
__device__ __forceinline__ constexpr int tile_first(const Geo&) { return 0; }
template <class Geo>
__device__ __forceinline__ constexpr int tile_end(const Geo&, int last) { return last; }
template <class Geo>
__device__ __forceinline__ constexpr float* out_base(const Geo&, float* O) { return O; }
template <class Geo>
__device__ __forceinline__ constexpr int out_slice(const Geo&, int b) { return b; }
template <class Geo>
__device__ __forceinline__ int tile_first(const Split<Geo>& g) { return g.first(); }
template <class Geo>
__device__ __forceinline__ int tile_end(const Split<Geo>& g, int last) { return min(last, g.end()); }
template <class Geo>
__device__ __forceinline__ float* out_base(const Split<Geo>& g, float*) { return g.Oc; }
template <class Geo>
__device__ __forceinline__ int out_slice(const Split<Geo>& g, int b) { return b * g.NC + g.c; }
// Window: the workgroup's sweep starts at its first stage; where a wave's own tiles start is first(qg), in the bodies
template <class Geo>
__device__ __forceinline__ int tile_first(const Window<Geo>& g) { return g.t0; }

// A geometry that also carries the buffers of a dumping instance (int8 kernel; QkDump and PDump in
// qmha_kernels.hpp): the debug hook's twin of a shipped instance, whose own arguments stay as they are.
template <class Geo>
struct Dumping : Geo {
    // the dump's arrays are indexed by the query slice b * h + k, which the kernel takes to be its K/V slice
    static_assert(!std::is_same<Geo, Grouped>::value, "the dump indexes by query slice: Grouped has no twin");
    static constexpr bool kDump = true;
    QkDump qk;
    PDump pd;
    Dumping(Geo g, QkDump q, PDump p) : Geo(g), qk(q), pd(p) {}
};

// Launch index -> (bh, q-block pair): a workgroup runs q-block nqb - 1 - pi and then its mirror pi, so every
// workgroup of a head costs the same nqb + 1 q-block units (the middle q-block of an odd nqb runs alone);
// consecutive indices of an XCD share (b, h), and the pairs holding the largest q-blocks start first.
// (int8 kernel.  The fp16 kernel keeps one q-block per workgroup, heaviest first -- masked_wg_single: with the
// pair loop around it its d = 64 instance no longer fits the 128 VGPRs of four waves per SIMD, 4 spilled, and
// it has no grid that is resident all at once among the measured shapes.)
__host__ __device__ constexpr int masked_pairs(int nqb) { return (nqb + 1) / 2; }
__device__ __forceinline__ void masked_wg_single(int nqb, int& bh, int& qb) {
    const int wg = xcd_remap(blockIdx.x, gridDim.x);
    bh = wg / nqb;
    qb = nqb - 1 - wg % nqb;
}
__device__ __forceinline__ void masked_wg(int nqb, int& bh, int& pi) {
    const int wg = xcd_remap(blockIdx.x, gridDim.x);
    bh = wg / masked_pairs(nqb);
    pi = wg % masked_pairs(nqb);
}
// Split: launch index -> (K/V slice, unit block, chunk); the chunks of a unit block are neighbours, so c < nc whatever
// the grid is, and xcd_remap keeps a K/V slice's workgroups on one XCD
__device__ __forceinline__ void split_wg(int nqb, int nc, int& bh, int& qb, int& c) {
    const unsigned wg = (unsigned)xcd_remap(blockIdx.x, gridDim.x), per = (unsigned)(nqb * nc);
    const unsigned r = wg % per;
    bh = (int)(wg / per);
    qb = (int)(r / (unsigned)nc);
    c = (int)(r % (unsigned)nc);
}

// K/V staging of both kernels: fixed per-lane source offsets (the LDS image's swizzle applied to the
// source address by the kernel that fills koff / voff), the stage offset in soffset.
template <int WAVES, int KCH, int VCH, int KBYTES, int VBYTES, int SG>
struct MaskedStager {
    static constexpr int KJ = (KCH / 64 + WAVES - 1) / WAVES, VJ = (VCH / 64 + WAVES - 1) / WAVES;
    int koff[KJ], voff[VJ];
    // ngr: tiles of the stage to bring in (1..SG, wave-uniform)
    __device__ __forceinline__ void issue(char* L, const char* kbase, int knrec, const char* vbase, int vnrec, int st,
                                          int ngr, int wave) const {
#pragma unroll
        for (int jj = 0; jj < KJ; ++jj) {
            const int inst = wave + jj * WAVES;
            if (inst < KCH / 64 && inst * 64 < ngr * (KCH / SG))
                buffer_load_lds16(kbase, knrec, (lptr_t)(L + inst * 1024), koff[jj], st * KBYTES);
        }
#pragma unroll
        for (int jj = 0; jj < VJ; ++jj) {
            const int inst = wave + jj * WAVES;
            if (inst < VCH / 64 && inst * 64 < ngr * (VCH / SG))
                buffer_load_lds16(vbase, vnrec, (lptr_t)(L + KBYTES + inst * 1024), voff[jj], st * VBYTES);
        }
    }
};

// A sequence with an invalid length (Varlen): the O rows of the workgroup's unit block qb are written as zeros, a
// wave per active unit; nothing is read.
template <int D>
__device__ __forceinline__ void zero_unit_block(float* __restrict__ O, const Varlen& geo, int bh, int H, int d_model, int qb) {
    constexpr int C4 = D / 4;
    const int lane = threadIdx.x & 63;
    const int u = qb * kWaves + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (u >= geo.units()) return;  // wave-uniform
    float* o = O + ((size_t)(bh / H) * geo.nq() + (size_t)geo.group(u) * QMHA_GROUP) * d_model + (size_t)geo.head(bh % H, u) * D;
#pragma unroll
    for (int i = lane; i < QMHA_GROUP * C4; i += 64) *reinterpret_cast<v4f*>(o + (size_t)(i / C4) * d_model + 4 * (i % C4)) = v4f{};
}

// A sequence with an invalid length (Ragged, Paged): its Nq real rows of O are zeroed by the first workgroup of each of
// its K/V slices -- the G heads' columns of those rows --, and nothing is read.
template <int D>
__device__ __forceinline__ void zero_real_rows(float* __restrict__ O, const Ragged& geo, int bh, int H, int d_model) {
    const int W4 = geo.G * D / 4;  // 16-byte pieces of a row's G heads
    float* o = O + (size_t)(bh / H) * geo.Nq * d_model + (size_t)(bh % H) * geo.G * D;
    for (int i = threadIdx.x; i < geo.Nq * W4; i += kWaves * 64) *reinterpret_cast<v4f*>(o + (size_t)(i / W4) * d_model + 4 * (i % W4)) = v4f{};
}

// ---------------------------------------------------------------------------------------
// The prologue of a packed sequence (Packed<Base>; text kept as it shipped: reworded inline it moved two int8 instances'
// bytes).  Workgroup-uniform (b is), before the body's first barrier or DMA issue:
//   range      0 <= cu[b] <= cu[b + 1] <= total, or nothing of the sequence is read or written: no address is formed
//   empty      cu[b + 1] == cu[b]: the sequence sits out, lens[b] is not looked at
//   invalid    nq_b > max_nq (the grid's bound: Nq of `any`), lens[b] outside [nq_b, cap], or (paged) a used table entry
//              outside the pool: rows [cu[b], cu[b + 1]) of O are positive zeros -- written by the first workgroup of each
//              K/V slice, its G heads' columns -- and none of the sequence's K/V is read
//   valid      the sequence's geometry is Ragged::of / Paged::of with Nq = nq_b, and its first row is cu[b]
// The two loads of cu are scalar loads of a wave-uniform address; readfirstlane keeps what follows in scalar registers.
// ---------------------------------------------------------------------------------------
struct PackedSeq {
    int row0, nq, L;
    int verdict;  // 0: leave, nothing written; 1: zero the rows and leave; 2: run the body
};
template <class Base>
__device__ __forceinline__ PackedSeq packed_seq(const Packed<Base>& any, const int32_t* __restrict__ lens, int b) {
    PackedSeq q{0, 0, 0, 0};
    const int r0 = __builtin_amdgcn_readfirstlane(any.cu[b]), r1 = __builtin_amdgcn_readfirstlane(any.cu[b + 1]);
    if (r0 < 0 || r1 < r0 || r1 > any.total) return q;  // the range never becomes an address
    if (r1 == r0) return q;                             // an empty sequence sits out
    q.row0 = r0, q.nq = r1 - r0, q.verdict = 1;
    if (q.nq > any.Nq) return q;  // beyond what the grid was sized for
    q.L = __builtin_amdgcn_readfirstlane(lens[b]);
    if (q.L < q.nq || q.L > any.Nk) return q;
    if constexpr (kPagedGeo<Base>) {
        if (!any.used_pages_ok(b, q.L)) return q;
    }
    q.verdict = 2;
    return q;
}
// rows [row0, row0 + nq) of O, the G heads' columns of K/V head kvh: in bounds by the range test
template <int D>
__device__ __forceinline__ void zero_packed_rows(float* __restrict__ O, const PackedSeq& q, int G, int kvh, int d_model) {
    const int W4 = G * D / 4;  // 16-byte pieces of a row's G heads
    float* o = O + (size_t)q.row0 * d_model + (size_t)kvh * G * D;
    for (int i = threadIdx.x; i < q.nq * W4; i += kWaves * 64) *reinterpret_cast<v4f*>(o + (size_t)(i / W4) * d_model + 4 * (i % W4)) = v4f{};
}

// ---------------------------------------------------------------------------------------
// The attend kernels of a persistent K/V cache: one template per precision over Geo = Ragged,
// Paged (instantiated in qmha_fa_masked.hip), Packed<Ragged> or Packed<Paged> (qmha_fa_packed.hip).  The prologue reads
// the sequence's words from device memory and gives its verdict -- workgroup-uniform (b is), before the body's first
// barrier or DMA issue -- and the same body runs over the geometry of that sequence.
//   cache_seq   Packed: packed_seq above.  Otherwise one scalar load of lens[b]; a length outside [Nq, cap], or (Paged) a
//               used table entry outside the pool, is verdict 1: the sequence's Nq rows of O are zeros, none of its K/V
//               is read.  These geometries have no verdict 0.
//   zero_seq_rows / seq_geo   the rows verdict 1 zeroes, and of() from what the prologue read
// ---------------------------------------------------------------------------------------
template <class Geo>
__device__ __forceinline__ PackedSeq cache_seq(const Geo& any, const int32_t* __restrict__ lens, int b) {
    if constexpr (kPackedGeo<Geo>) return packed_seq(any, lens, b);
    else {
        const int L = lens[b];
        PackedSeq q{0, any.Nq, L, 1};
        if (!any.valid(L)) return q;
        if constexpr (kPagedGeo<Geo>) {
            if (!any.used_pages_ok(b, L)) return q;
        }
        q.verdict = 2;
        return q;
    }
}
template <int D, class Geo>
__device__ __forceinline__ void zero_seq_rows(float* __restrict__ O, const Geo& any, const PackedSeq& q, int bh, int H, int d_model) {
    if constexpr (kPackedGeo<Geo>) zero_packed_rows<D>(O, q, any.G, bh % H, d_model);
    else zero_real_rows<D>(O, any, bh, H, d_model);
}
template <class Geo>
__device__ __forceinline__ Geo seq_geo(const Geo& any, const PackedSeq& q) {
    if constexpr (kPackedGeo<Geo>) return any.of(q.row0, q.nq, q.L);
    else return any.of(q.L);
}

// (int8 d = 32 asks for the seven waves per SIMD its varlen sibling has: under the shared bound of four the row shift
// took it from 68 to 75 VGPRs, one occupancy step; with seven it needs 70 and no scratch.)
template <int D, class Geo>
__global__ __launch_bounds__(kWaves * 64, D > 64 ? 2 : D > 32 ? 4 : 7) void qmha_fa_int8_cache_kernel(
    const float* __restrict__ Qf, const int8_t* __restrict__ Ki, const _Float16* __restrict__ Vh,
    const float* __restrict__ sK, const float* __restrict__ sV, float* __restrict__ O, Geo any,
    const int32_t* __restrict__ lens, int H, int d_model, int nqb, float c_log2) {
    int bh_, pi_;
    masked_wg(nqb, bh_, pi_);  // the body forms the same pair again
    const PackedSeq q = cache_seq(any, lens, bh_ / H);
    if (q.verdict != 2) {
        if (q.verdict == 1 && pi_ == 0) zero_seq_rows<D>(O, any, q, bh_, H, d_model);
        return;
    }
    const Geo geo = seq_geo(any, q);
#include "qmha_fa_masked_int8.inc"
}

template <int D, class Geo>
__global__ __launch_bounds__(kWaves * 64, D > 64 ? 2 : 4) void qmha_fa_f16_cache_kernel(
    const float* __restrict__ Qf, const _Float16* __restrict__ Kh, const _Float16* __restrict__ Vt,
    float* __restrict__ O, Geo any, const int32_t* __restrict__ lens, int H, int d_model, int nqb, float c_log2) {
    int bh_, qb_;
    masked_wg_single(nqb, bh_, qb_);  // the body forms the same pair again
    const PackedSeq q = cache_seq(any, lens, bh_ / H);
    if (q.verdict != 2) {
        if (q.verdict == 1 && qb_ == 0) zero_seq_rows<D>(O, any, q, bh_, H, d_model);
        return;
    }
    const Geo geo = seq_geo(any, q);
#include "qmha_fa_masked_f16.inc"
}

// ---------------------------------------------------------------------------------------
// host: the geometry of a call (MaskedCall in qmha_kernels.hpp).  Token-granular lengths take Ragged (a table: Paged),
// per-sequence lengths Varlen, grouped calls (Hkv < H) Grouped, square causal calls of their own SquareCausal,
// everything else Rect
// ---------------------------------------------------------------------------------------
static bool masked_shape_ok(int Nq, int Nk, bool causal) {
    return Nq >= QMHA_GROUP && Nk >= QMHA_GROUP && Nq % QMHA_GROUP == 0 && Nk % QMHA_GROUP == 0 && !(causal && Nk < Nq);
}
// K/V cache: a cache of `cap` rows of which `len` are valid, Nk = cap.  causal: Rect::cached; else
// every row attends all cap rows, so len == cap.
static bool cached_shape_ok(int Nq, int cap, int len, bool causal) {
    if (!masked_shape_ok(Nq, cap, false) || len % QMHA_GROUP != 0) return false;
    return causal ? Nq <= len && len <= cap : len == cap;
}
static int masked_nqb(int units) { return (units + kWaves - 1) / kWaves; }  // unit blocks per K/V slice
// the units a grid is sized for: the geometry's own, or, where they follow a length on the device (Ragged), their most
template <class Geo>
static int grid_units(const Geo& geo) {
    if constexpr (std::is_base_of<Ragged, Geo>::value) return geo.max_units();
    else return geo.units();
}

// The geometry of a call, checked, handed to `launch`.  The varlen grid follows Nq, B, Hkv and G only; what lens
// holds is the kernels' business.
template <class Launch>
static hipError_t masked_geo(const MaskedCall& c, Launch&& launch) {
    if (c.B < 1 || c.Hkv < 1 || c.Hkv > c.H || c.H % c.Hkv != 0 || c.d_model != c.H * c.D) return hipErrorInvalidValue;
    if (c.ragged) {  // token-granular lengths: any 1 <= Nq <= cap, causal, lengths on the device
        if (!c.lens || !c.causal || c.Nq < 1 || c.Nk < QMHA_GROUP || c.Nk % QMHA_GROUP != 0 || c.Nq > c.Nk) return hipErrorInvalidValue;
        const Ragged r(c.Nq, c.Nk, c.H / c.Hkv);
        const PageTable& p = c.pages;
        if (!p.table) return launch(r);
        // a paged cache: Nk is the logical capacity max_pages * page_rows (an int), w the pool's carve
        if (p.page_rows < 2 * QMHA_GROUP || p.page_rows % (2 * QMHA_GROUP) != 0 || p.max_pages < 1 || p.num_pages < 1 ||
            (long long)p.max_pages * p.page_rows != c.Nk)
            return hipErrorInvalidValue;
        return launch(Paged(r, p.table, p.page_rows, p.max_pages, p.num_pages));
    }
    const bool cached = !c.lens && c.len >= 0;
    if (!(cached ? cached_shape_ok(c.Nq, c.Nk, c.len, c.causal) : masked_shape_ok(c.Nq, c.Nk, c.causal))) return hipErrorInvalidValue;
    const int G = c.H / c.Hkv;
    if (c.lens) return launch(Varlen(c.Nq, c.Nk, G, c.causal));
    if (!cached && G == 1 && c.causal && c.Nq == c.Nk) return launch(SquareCausal{c.Nq});
    const Rect r = cached && c.causal ? Rect::cached(c.Nq, c.Nk, c.len) : Rect(c.Nq, c.Nk, c.causal);
    return G > 1 ? launch(Grouped(r, G)) : launch(r);
}

}  // namespace qmha
