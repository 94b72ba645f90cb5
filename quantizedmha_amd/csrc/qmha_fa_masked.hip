// qmha_fa_masked.hip -- the main kernels of the int8 and fp16 fused attention paths that visit a masked or
// partial set of key tiles, for gfx950 (MI355X): square causal (is_causal=True),
// rectangular (Nq != Nk: cross-attention and chunked prefill) and grouped-query (h query
// heads on h_kv < h K/V heads).  One int8 and one fp16 kernel template; a compile-time
// geometry type (SquareCausal, Rect, Grouped: qmha_fa_masked.hpp) supplies what differs.  And the varlen kernels of a
// K/V cache whose sequences differ in length: the same body -- it is the text of
// qmha_fa_masked_{int8,f16}.inc, included by every __global__ here -- over a geometry (Varlen) formed from a length
// the kernel reads from device memory.  And the cache kernels (qmha_fa_{int8,f16}_cache_kernel, defined in the header):
// that body once more, over lengths and query counts that are no multiple of 32 (Ragged) and over a pool
// of pages, each stage's K/V found through a block table on the device (Paged).
// The split-KV kernels run the same bodies over Split<Ragged> / Split<Paged> from qmha_fa_split.hip; the
// packed-batch calls are the cache kernels over Packed<Ragged> / Packed<Paged>, instantiated in
// qmha_fa_packed.hip.  Geometries, stager and the checked geometry of a call are the header's.
//
// Square causal: query row r attends keys j <= r of its own sequence (Nq = Nk = N).  Both kernels keep the
// geometry of the non-causal main kernels, so they consume the unchanged pre-pass outputs (qmha_prepass.hip):
//   one wave = one 32-row query group g, a workgroup of 4 groups shares the LDS-DMA K/V staging
//   (buffer_load ... lds, stages of 2 key tiles, double-buffered), tiles are 32 keys wide.
//   group g visits key tiles t = 0..g; on the diagonal tile t == g a score with j > r is -inf BEFORE the
//   row maximum is formed: no part in the row max, p = 0 exactly, nothing in the row sum, (int8) Pi = 0 and
//   nothing in the P-tile absmax.
//   The workgroup's KV loop ends at the stage that holds its last wave's diagonal tile; later stages are
//   neither staged nor computed.  A wave whose diagonal lies earlier keeps taking part in every barrier
//   and every DMA issue and skips the tile body under a wave-uniform branch (it adds exactly zero).
//   The mask is one select per score under a wave-uniform branch taken on the diagonal tile only, so
//   off-diagonal tiles execute no mask instructions.  (A separate compile-time instantiation of the whole
//   tile body for the diagonal doubled the unrolled loop body and spilled -- fp16 d = 64: 221 VGPRs to
//   scratch at the 4-waves-per-SIMD budget -- so the tile body exists once.)
//   Workgroup cost grows with the q-block index.  fp16: the launch index maps the largest q-blocks of every
//   (b, h) first.  int8: a workgroup runs a PAIR of q-blocks one after the other,
//   nqb - 1 - i and its mirror i: every workgroup of a head then costs the same nqb + 1 units, whatever
//   compute unit it lands on (with heaviest-first single q-blocks, a grid that is resident all at once --
//   B1 H32 N8192 d32 -- ended 1.5x later than its mean: DESIGN.md 10).  The pairs with the largest
//   q-blocks start first; xcd_remap keeps the pairs of one (b, h) in one XCD's L2.
// Rectangular: Q and O are [B, Nq, d_model], K and V [B, Nk, d_model]; Gq = Nq / 32 query groups, Gk = Nk / 32
// key tiles.  The pre-pass touches K and V only and runs unchanged with N = Nk.  Query rows, O rows and `active`
// follow Gq; the K/V bases, the buffer extents, the sK / sV index and the loop bounds follow Gk.
//   diag_off (run-time, wave-uniform, SGPR) is the one switch between the two modes, so each kernel has one
//   rectangular instance per head size:
//     causal, bottom-right aligned (row r attends keys j <= r + Nk - Nq, Nk >= Nq): diag_off = Gk - Gq.  The
//       32-row K/V groups are aligned to the tile grid and Nk - Nq is a multiple of 32, so group g's diagonal
//       tile is exactly key tile g + diag_off and the in-tile mask is the square one (j > r inside the tile);
//       tiles past the diagonal are not visited.
//     non-causal: diag_off = Gk, a diagonal no tile reaches (t <= Gk - 1 < g + Gk): every wave runs all Gk
//       tiles and never takes the mask branch.
//   A wave's last tile is min(g + diag_off, Gk - 1); the workgroup's KV loop ends at the stage holding the last
//   tile of its last active wave, and the partial last stage brings in that many tiles only.  With an offset
//   every int8 workgroup of a head still costs the same; without the mask both passes cost Gk tiles.
// Grouped: Q and O are [B, Nq, h * D], K and V [B, Nk, h_kv * D], G = h / h_kv; the pre-pass runs unchanged with
// H = h_kv, so the workspace holds B * h_kv slices of Nk rows.  The rows, the diagonal and the cached form are Rect's.
//   K/V slice.  The launch index's slice is the K/V slice bh = b * h_kv + kvh (the kernels' H argument is the number
//     of K/V heads, which is h for the other geometries): the K/V bases, the buffer extents and the sK / sV index
//     use it; query rows and O rows keep d_model = h * D and column k * D of query head k.
//   Units.  One K/V slice serves U = G * Gq units: unit u = qg * G + j is query group qg of query head
//     kvh * G + j.  A workgroup holds four consecutive units (nqb = ceil(U / 4)); a wave is active when u < U;
//     diag and last take qg = u / G.  qg is non-decreasing in u, so the workgroup's last tile is that of its last
//     active unit.  With G = 4 a workgroup is the four heads of one query group: one shared diagonal, no wave
//     idle under the mask (decode, Nq = 32: four active waves per workgroup where Rect has one).  G is a
//     run-time, wave-uniform argument (any G >= 2).  For SquareCausal and Rect a unit is a query group of the
//     slice's own head: U = Gq, qg = u, k = kvh.
//   Grid.  B * h_kv * masked_pairs(nqb) for int8 (mirrored unit-block pairs), B * h_kv * nqb for fp16 (heaviest
//     first); xcd_remap keeps the workgroups of one K/V slice on one XCD, so the G heads re-read K/V from its L2.
//   A wave's arithmetic and tile order are those of the Rect instance, so a query head's result is that of the
//   multi-head call on K / V expanded G times, bit for bit.
// Out of range by construction: K/V reads go through buffer descriptors of exactly the (b, kvh) slice
// (Nk * D, Nk * 2D bytes) and a stage issues whole tiles t <= Gk - 1 only; sK / sV are read at t <= Gk - 1
// of slice bh * Gk; Q and O rows are touched by active waves only (u < U: qg < Gq, query head < h).
//
// int8 (fa_tc_int8_b contract): the tile of qmha_fa_int8_kernel -- i8 MFMA for Q@K^T, exact-integer f16
//   MFMA for P@V, one sP per 32x32 tile, the anchored O / l state -- on the Ki / Vh / sK / sV workspace.
// fp16 (fa_tc_v1a contract): the tile of qmha_fa_f16_v3_kernel -- v_mfma_f32_16x16x32_f16 for both
//   products, the lazy base of DESIGN.md 3 -- on the Kh / Vt workspace.
// Both are unpipelined (one tile at a time, co-resident waves interleave); N = 32 is the same kernel
// (one stage, one diagonal tile).
#include "qmha_fa_masked.hpp"

namespace qmha {

// ---------------------------------------------------------------------------------------
// int8: 32x32 accumulator map.  Lane (col, half) holds S^T[acc_row(r, half)][col], r = 0..15: query
// row `col` of the group against key acc_row(r, half) of the tile, so on the diagonal tile (the groups of
// queries and keys aligned) the score of register r is masked when acc_row(r, half) > col.
// ---------------------------------------------------------------------------------------
template <int D, class Geo>
__global__ __launch_bounds__(kWaves * 64, D > 64 ? 2 : 4) void qmha_fa_int8_masked_kernel(
    const float* __restrict__ Qf, const int8_t* __restrict__ Ki, const _Float16* __restrict__ Vh,
    const float* __restrict__ sK, const float* __restrict__ sV, float* __restrict__ O, Geo geo, int H, int d_model,
    int nqb, float c_log2) {
#include "qmha_fa_masked_int8.inc"
}

// Per-sequence lengths (Varlen, above): one scalar load of lens[b], then the same body over that sequence's geometry.
// An invalid length is a workgroup-uniform choice (b is), taken before the body's first barrier.
// (Geo is a template argument so that the body's `if constexpr (Geo::kDump)` branches are discarded unchecked.)
template <int D, class Geo = Varlen>
__global__ __launch_bounds__(kWaves * 64, D > 64 ? 2 : 4) void qmha_fa_int8_varlen_kernel(
    const float* __restrict__ Qf, const int8_t* __restrict__ Ki, const _Float16* __restrict__ Vh,
    const float* __restrict__ sK, const float* __restrict__ sV, float* __restrict__ O, Geo any,
    const int32_t* __restrict__ lens, int H, int d_model, int nqb, float c_log2) {
    int bh_, pi_;
    masked_wg(nqb, bh_, pi_);  // the body forms the same pair again
    const int L = lens[bh_ / H];
    if (!any.valid(L)) {
        zero_unit_block<D>(O, any, bh_, H, d_model, nqb - 1 - pi_);
        if (pi_ != nqb - 1 - pi_) zero_unit_block<D>(O, any, bh_, H, d_model, pi_);
        return;
    }
    const Geo geo = any.of(L);
#include "qmha_fa_masked_int8.inc"
}

// ---------------------------------------------------------------------------------------
// fp16: 16x16 accumulator map (qmha_fa_f16_v3_kernel).  Lane l = 16 grp + r16 holds, per query block
// qb, S^T[kap16(kb, 4 grp + i)][16 qb + r16] (kb = 0, 1, i = 0..3): on the diagonal tile that score
// is masked when kap16(kb, 4 grp + i) > 16 qb + r16.
// ---------------------------------------------------------------------------------------
template <int D, class Geo>
__global__ __launch_bounds__(kWaves * 64, D > 64 ? 2 : 4) void qmha_fa_f16_masked_kernel(
    const float* __restrict__ Qf, const _Float16* __restrict__ Kh, const _Float16* __restrict__ Vt,
    float* __restrict__ O, Geo geo, int H, int d_model, int nqb, float c_log2) {
#include "qmha_fa_masked_f16.inc"
}

// Per-sequence lengths, as qmha_fa_int8_varlen_kernel
template <int D>
__global__ __launch_bounds__(kWaves * 64, D > 64 ? 2 : 4) void qmha_fa_f16_varlen_kernel(
    const float* __restrict__ Qf, const _Float16* __restrict__ Kh, const _Float16* __restrict__ Vt,
    float* __restrict__ O, Varlen any, const int32_t* __restrict__ lens, int H, int d_model, int nqb, float c_log2) {
    int bh_, qb_;
    masked_wg_single(nqb, bh_, qb_);  // the body forms the same pair again
    const int L = lens[bh_ / H];
    if (!any.valid(L)) {
        zero_unit_block<D>(O, any, bh_, H, d_model, qb_);
        return;
    }
    const auto geo = as_dependent<D>(any.of(L));
#include "qmha_fa_masked_f16.inc"
}

// ---------------------------------------------------------------------------------------
// host launchers (MaskedCall in qmha_kernels.hpp; masked_geo picks the geometry): a persistent cache (Ragged, Paged)
// takes the cache kernels, per-sequence lengths the varlen kernels, every other geometry the masked templates
// ---------------------------------------------------------------------------------------
// Launch the instance of `geo` over the call's B * Hkv K/V slices (the kernels' H argument); stream: the dump's is null
template <class Geo>
static hipError_t fa_masked_launch(const Int8Workspace& w, const float* Qf, float* O, const MaskedCall& c, hipStream_t stream, Geo geo) {
    const int nqb = masked_nqb(grid_units(geo));
    const dim3 grid(c.B * c.Hkv * masked_pairs(nqb)), block(kWaves * 64);
    return int8_masked_d(c.D, [&](auto d) {
        if constexpr (kRaggedGeo<Geo>)  // Ragged, Paged: a persistent cache
            hipLaunchKernelGGL((qmha_fa_int8_cache_kernel<decltype(d)::value, Geo>), grid, block, 0, stream, Qf, w.Ki, w.Vh, w.sK, w.sV, O,
                               geo, c.lens, c.Hkv, c.d_model, nqb, softmax_scale_log2(c.D));
        else if constexpr (std::is_same<Geo, Varlen>::value)
            hipLaunchKernelGGL((qmha_fa_int8_varlen_kernel<decltype(d)::value>), grid, block, 0, stream, Qf, w.Ki, w.Vh, w.sK, w.sV, O,
                               geo, c.lens, c.Hkv, c.d_model, nqb, softmax_scale_log2(c.D));
        else
            hipLaunchKernelGGL((qmha_fa_int8_masked_kernel<decltype(d)::value, Geo>), grid, block, 0, stream, Qf, w.Ki, w.Vh, w.sK,
                               w.sV, O, geo, c.Hkv, c.d_model, nqb, softmax_scale_log2(c.D));
        return hipGetLastError();
    });
}

template <class Geo>
static hipError_t fa_masked_launch(const F16Workspace& w, const float* Qf, float* O, const MaskedCall& c, hipStream_t stream, Geo geo) {
    const int nqb = masked_nqb(grid_units(geo));
    const dim3 grid(c.B * c.Hkv * nqb), block(kWaves * 64);
    return f16_masked_d(c.D, [&](auto d) {
        if constexpr (kRaggedGeo<Geo>)
            hipLaunchKernelGGL((qmha_fa_f16_cache_kernel<decltype(d)::value, Geo>), grid, block, 0, stream, Qf, w.Kh, w.Vt, O, geo, c.lens,
                               c.Hkv, c.d_model, nqb, softmax_scale_log2(c.D));
        else if constexpr (std::is_same<Geo, Varlen>::value)
            hipLaunchKernelGGL((qmha_fa_f16_varlen_kernel<decltype(d)::value>), grid, block, 0, stream, Qf, w.Kh, w.Vt, O, geo, c.lens,
                               c.Hkv, c.d_model, nqb, softmax_scale_log2(c.D));
        else
            hipLaunchKernelGGL((qmha_fa_f16_masked_kernel<decltype(d)::value, Geo>), grid, block, 0, stream, Qf, w.Kh, w.Vt, O, geo,
                               c.Hkv, c.d_model, nqb, softmax_scale_log2(c.D));
        return hipGetLastError();
    });
}

// The instances of this file, in the order they stand in its code object (kernels are emitted as they are
// instantiated).  The order is part of the shipped bytes: the dumping twins reach their out-of-line dump lambdas
// PC-relative, so what stands before them shows in their code (isa_id).
#define QMHA_INSTANCE(W, ...) \
    template hipError_t fa_masked_launch<__VA_ARGS__>(const W&, const float*, float*, const MaskedCall&, hipStream_t, __VA_ARGS__);
QMHA_INSTANCE(Int8Workspace, SquareCausal)
QMHA_INSTANCE(Int8Workspace, Dumping<SquareCausal>)
QMHA_INSTANCE(Int8Workspace, Dumping<Rect>)
QMHA_INSTANCE(F16Workspace, SquareCausal)
QMHA_INSTANCE(Int8Workspace, Rect)
QMHA_INSTANCE(F16Workspace, Rect)
QMHA_INSTANCE(Int8Workspace, Grouped)
QMHA_INSTANCE(F16Workspace, Grouped)
QMHA_INSTANCE(Int8Workspace, Varlen)
QMHA_INSTANCE(F16Workspace, Varlen)
QMHA_INSTANCE(Int8Workspace, Ragged)
QMHA_INSTANCE(F16Workspace, Ragged)
QMHA_INSTANCE(Int8Workspace, Paged)
QMHA_INSTANCE(F16Workspace, Paged)
#undef QMHA_INSTANCE

hipError_t launch_fa_masked(const Int8Workspace& w, const float* Qf, float* O, const MaskedCall& c, hipStream_t stream) {
    return masked_geo(c, [&](auto geo) { return fa_masked_launch(w, Qf, O, c, stream, geo); });
}

hipError_t launch_fa_masked(const F16Workspace& w, const float* Qf, float* O, const MaskedCall& c, hipStream_t stream) {
    return masked_geo(c, [&](auto geo) { return fa_masked_launch(w, Qf, O, c, stream, geo); });
}

// The dumping twin of the instance launch_fa_masked launches: the same grid and arguments, the geometry wrapped in
// Dumping<>, which the grouped and varlen geometries do not have
hipError_t launch_fa_int8_masked_pstage_dump(const Int8Workspace& w, const float* Qf, float* O, const MaskedCall& c, QkDump dbg,
                                             PDump pd) {
    return masked_geo(c, [&](auto geo) {
        if constexpr (std::is_base_of<Grouped, decltype(geo)>::value) return hipErrorInvalidValue;
        else return fa_masked_launch(w, Qf, O, c, nullptr, Dumping<decltype(geo)>(geo, dbg, pd));
    });
}

}  // namespace qmha
