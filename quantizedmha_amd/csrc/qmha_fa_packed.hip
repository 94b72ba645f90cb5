// qmha_fa_packed.hip -- packed batches for the token-granular and paged attends of a K/V cache, for
// gfx950 (MI355X): Q and O are [total, d_model] with no batch axis, and a device array int32 cu[B + 1] gives sequence b
// the rows [cu[b], cu[b + 1]) -- a query count of its own per sequence, read when the kernel runs.  The kernels are the
// bodies of qmha_fa_masked.hip's kernels once more (qmha_fa_masked_{int8,f16}.inc), over Packed<Ragged> and
// Packed<Paged>; the geometries, the stager and masked_geo are that file's text, included without its kernels (a
// translation unit of its own for the reason qmha_fa_split.hip is one).
#define QMHA_FA_SPLIT_TU
#include "qmha_fa_masked.hip"

namespace qmha {

// ---------------------------------------------------------------------------------------
// The prologue of every packed kernel.  Workgroup-uniform (b is), before the body's first barrier or DMA issue:
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

// The launch bounds are the ragged / paged siblings' (int8 d = 32 asks for their seven waves per SIMD)
template <int D, class Base = Ragged>
__global__ __launch_bounds__(kWaves * 64, D > 64 ? 2 : D > 32 ? 4 : 7) void qmha_fa_int8_packed_kernel(
    const float* __restrict__ Qf, const int8_t* __restrict__ Ki, const _Float16* __restrict__ Vh,
    const float* __restrict__ sK, const float* __restrict__ sV, float* __restrict__ O, Packed<Base> any,
    const int32_t* __restrict__ lens, int H, int d_model, int nqb, float c_log2) {
    using Geo = Packed<Base>;
    int bh_, pi_;
    masked_wg(nqb, bh_, pi_);  // the body forms the same pair again
    const PackedSeq q = packed_seq(any, lens, bh_ / H);
    if (q.verdict != 2) {  // workgroup-uniform, before the body's first barrier
        if (q.verdict == 1 && pi_ == 0) zero_packed_rows<D>(O, q, any.G, bh_ % H, d_model);
        return;
    }
    const Geo geo = any.of(q.row0, q.nq, q.L);
#include "qmha_fa_masked_int8.inc"
}

template <int D, class Base = Ragged>
__global__ __launch_bounds__(kWaves * 64, D > 64 ? 2 : 4) void qmha_fa_f16_packed_kernel(
    const float* __restrict__ Qf, const _Float16* __restrict__ Kh, const _Float16* __restrict__ Vt,
    float* __restrict__ O, Packed<Base> any, const int32_t* __restrict__ lens, int H, int d_model, int nqb, float c_log2) {
    using Geo = Packed<Base>;
    int bh_, qb_;
    masked_wg_single(nqb, bh_, qb_);  // the body forms the same pair again
    const PackedSeq q = packed_seq(any, lens, bh_ / H);
    if (q.verdict != 2) {
        if (q.verdict == 1 && qb_ == 0) zero_packed_rows<D>(O, q, any.G, bh_ % H, d_model);
        return;
    }
    const Geo geo = any.of(q.row0, q.nq, q.L);
#include "qmha_fa_masked_f16.inc"
}

// A paged cache: the same two kernels under names of their own, as the ragged and the paged kernels are (every kernel
// template of the library has one instance per head size)
template <int D, class Base = Paged>
__global__ __launch_bounds__(kWaves * 64, D > 64 ? 2 : D > 32 ? 4 : 7) void qmha_fa_int8_packed_pages_kernel(
    const float* __restrict__ Qf, const int8_t* __restrict__ Ki, const _Float16* __restrict__ Vh,
    const float* __restrict__ sK, const float* __restrict__ sV, float* __restrict__ O, Packed<Base> any,
    const int32_t* __restrict__ lens, int H, int d_model, int nqb, float c_log2) {
    using Geo = Packed<Base>;
    int bh_, pi_;
    masked_wg(nqb, bh_, pi_);  // the body forms the same pair again
    const PackedSeq q = packed_seq(any, lens, bh_ / H);
    if (q.verdict != 2) {
        if (q.verdict == 1 && pi_ == 0) zero_packed_rows<D>(O, q, any.G, bh_ % H, d_model);
        return;
    }
    const Geo geo = any.of(q.row0, q.nq, q.L);
#include "qmha_fa_masked_int8.inc"
}

template <int D, class Base = Paged>
__global__ __launch_bounds__(kWaves * 64, D > 64 ? 2 : 4) void qmha_fa_f16_packed_pages_kernel(
    const float* __restrict__ Qf, const _Float16* __restrict__ Kh, const _Float16* __restrict__ Vt,
    float* __restrict__ O, Packed<Base> any, const int32_t* __restrict__ lens, int H, int d_model, int nqb, float c_log2) {
    using Geo = Packed<Base>;
    int bh_, qb_;
    masked_wg_single(nqb, bh_, qb_);  // the body forms the same pair again
    const PackedSeq q = packed_seq(any, lens, bh_ / H);
    if (q.verdict != 2) {
        if (q.verdict == 1 && qb_ == 0) zero_packed_rows<D>(O, q, any.G, bh_ % H, d_model);
        return;
    }
    const Geo geo = any.of(q.row0, q.nq, q.L);
#include "qmha_fa_masked_f16.inc"
}

// The grid is Ragged's at Nq = max_nq: a sequence of nq_b <= max_nq rows has at most ceil((nq_b + 31) / 32) active
// groups, no more than max_units() / G
template <class Geo>
static hipError_t fa_packed_launch(const Int8Workspace& w, const float* Qf, float* O, const MaskedCall& c, const int32_t* cu, int total,
                                   hipStream_t stream, Geo geo) {
    const int nqb = masked_nqb(grid_units(geo));
    if ((long long)c.B * c.Hkv * masked_pairs(nqb) > 0x7fffffffLL) return hipErrorInvalidValue;
    const Packed<Geo> pg(geo, cu, total);
    const dim3 grid(c.B * c.Hkv * masked_pairs(nqb)), block(kWaves * 64);
    return int8_masked_d(c.D, [&](auto d) {
        if constexpr (kPagedGeo<Geo>)
            hipLaunchKernelGGL((qmha_fa_int8_packed_pages_kernel<decltype(d)::value>), grid, block, 0, stream, Qf, w.Ki, w.Vh, w.sK, w.sV, O,
                               pg, c.lens, c.Hkv, c.d_model, nqb, softmax_scale_log2(c.D));
        else
            hipLaunchKernelGGL((qmha_fa_int8_packed_kernel<decltype(d)::value>), grid, block, 0, stream, Qf, w.Ki, w.Vh, w.sK, w.sV, O, pg,
                               c.lens, c.Hkv, c.d_model, nqb, softmax_scale_log2(c.D));
        return hipGetLastError();
    });
}

template <class Geo>
static hipError_t fa_packed_launch(const F16Workspace& w, const float* Qf, float* O, const MaskedCall& c, const int32_t* cu, int total,
                                   hipStream_t stream, Geo geo) {
    const int nqb = masked_nqb(grid_units(geo));
    if ((long long)c.B * c.Hkv * nqb > 0x7fffffffLL) return hipErrorInvalidValue;
    const Packed<Geo> pg(geo, cu, total);
    const dim3 grid(c.B * c.Hkv * nqb), block(kWaves * 64);
    return f16_masked_d(c.D, [&](auto d) {
        if constexpr (kPagedGeo<Geo>)
            hipLaunchKernelGGL((qmha_fa_f16_packed_pages_kernel<decltype(d)::value>), grid, block, 0, stream, Qf, w.Kh, w.Vt, O, pg, c.lens,
                               c.Hkv, c.d_model, nqb, softmax_scale_log2(c.D));
        else
            hipLaunchKernelGGL((qmha_fa_f16_packed_kernel<decltype(d)::value>), grid, block, 0, stream, Qf, w.Kh, w.Vt, O, pg, c.lens, c.Hkv,
                               c.d_model, nqb, softmax_scale_log2(c.D));
        return hipGetLastError();
    });
}

// The instances of this file, in the order they stand in its code object
#define QMHA_PACKED_INSTANCE(W, G) \
    template hipError_t fa_packed_launch<G>(const W&, const float*, float*, const MaskedCall&, const int32_t*, int, hipStream_t, G);
QMHA_PACKED_INSTANCE(Int8Workspace, Ragged)
QMHA_PACKED_INSTANCE(F16Workspace, Ragged)
QMHA_PACKED_INSTANCE(Int8Workspace, Paged)
QMHA_PACKED_INSTANCE(F16Workspace, Paged)
#undef QMHA_PACKED_INSTANCE

template <class W>
static hipError_t packed_any(const W& w, const float* Qf, float* O, const MaskedCall& c, const int32_t* cu, int total, hipStream_t stream) {
    if (!c.ragged || !cu || total < 1 || c.Nq > total) return hipErrorInvalidValue;
    return masked_geo(c, [&](auto geo) {
        if constexpr (kRaggedGeo<decltype(geo)>) return fa_packed_launch(w, Qf, O, c, cu, total, stream, geo);
        else return hipErrorInvalidValue;
    });
}
hipError_t launch_fa_packed(const Int8Workspace& w, const float* Qf, float* O, const MaskedCall& c, const int32_t* cu, int total,
                            hipStream_t stream) {
    return packed_any(w, Qf, O, c, cu, total, stream);
}
hipError_t launch_fa_packed(const F16Workspace& w, const float* Qf, float* O, const MaskedCall& c, const int32_t* cu, int total,
                            hipStream_t stream) {
    return packed_any(w, Qf, O, c, cu, total, stream);
}

}  // namespace qmha
