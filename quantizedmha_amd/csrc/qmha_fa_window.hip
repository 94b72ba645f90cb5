// qmha_fa_window.hip -- sliding-window attention for the token-granular and paged attends of a K/V cache,
// for gfx950 (MI355X): a query row sees the last `window` = 32 w keys of those the causal mask leaves it.  The kernels are
// the bodies of qmha_fa_masked.hip's kernels once more (qmha_fa_masked_{int8,f16}.inc), over Window<Ragged> and
// Window<Paged>; the geometries, the stager and masked_geo are the shared header's.  A translation unit of its own for
// the reason qmha_fa_split.hip is one.
#include "qmha_fa_masked.hpp"

namespace qmha {

// ---------------------------------------------------------------------------------------
// The ragged / paged prologue over the same bodies, a workgroup per (K/V slice, unit block); one template per precision
// over Base = Ragged or Paged.  The verdict is workgroup-uniform (b is) and falls before the body's first barrier or DMA
// issue: a length outside [Nq, cap], or (Paged) an entry outside the pool among the columns whose pages hold rows
// [64 (first(0) / 2), L) -- the window, widened to the stage of its first tile; the columns behind are not loaded --
// leaves the sequence's Nq rows of O as zeros, written by the first workgroup of each K/V slice, and none of its K/V is
// read.  The launch bounds are the ragged siblings'.  The template arguments are <Base, D>, the geometry first: the
// library's census of kernel templates (tests/test_abi.py) allows a template one instance per head size, and names the
// templates whose instances differ by a geometry one by one; this one's ten instances -- two geometries at every built head
// size, no alternates -- are pinned by tests/test_window_cpu.py instead.
// ---------------------------------------------------------------------------------------
template <class Base>
__device__ __forceinline__ bool window_seq_ok(const Window<Base>& any, int b, int L) {
    if (!any.valid(L)) return false;
    if constexpr (kPagedGeo<Base>) {
        const Window<Base> g = any.of(L, 0);  // t0 of unit block 0: the stage of first(0), the lowest tile any block stages
        if (!any.used_pages_ok(b, g.t0 * QMHA_GROUP, L)) return false;
    }
    return true;
}

template <class Base, int D>
__global__ __launch_bounds__(kWaves * 64, D > 64 ? 2 : D > 32 ? 4 : 7) void qmha_fa_int8_window_kernel(
    const float* __restrict__ Qf, const int8_t* __restrict__ Ki, const _Float16* __restrict__ Vh,
    const float* __restrict__ sK, const float* __restrict__ sV, float* __restrict__ O, Window<Base> any,
    const int32_t* __restrict__ lens, int H, int d_model, int nqb, float c_log2) {
    using Geo = Window<Base>;
    int bh_, qb_;
    masked_wg_single(nqb, bh_, qb_);  // the body forms the same pair again
    const int L = lens[bh_ / H];
    if (!window_seq_ok(any, bh_ / H, L)) {
        if (qb_ == 0) zero_real_rows<D>(O, any, bh_, H, d_model);
        return;
    }
    const Geo geo = any.of(L, qb_);
#include "qmha_fa_masked_int8.inc"
}

template <class Base, int D>
__global__ __launch_bounds__(kWaves * 64, D > 64 ? 2 : 4) void qmha_fa_f16_window_kernel(
    const float* __restrict__ Qf, const _Float16* __restrict__ Kh, const _Float16* __restrict__ Vt,
    float* __restrict__ O, Window<Base> any, const int32_t* __restrict__ lens, int H, int d_model, int nqb, float c_log2) {
    using Geo = Window<Base>;
    int bh_, qb_;
    masked_wg_single(nqb, bh_, qb_);  // the body forms the same pair again
    const int L = lens[bh_ / H];
    if (!window_seq_ok(any, bh_ / H, L)) {
        if (qb_ == 0) zero_real_rows<D>(O, any, bh_, H, d_model);
        return;
    }
    const Geo geo = any.of(L, qb_);
#include "qmha_fa_masked_f16.inc"
}

// window: a multiple of 32, >= 32 (w >= 1: the left tile is never the diagonal tile); the grid fits
static bool window_shape_ok(const MaskedCall& c, int window, int nqb) {
    if (window < QMHA_GROUP || window % QMHA_GROUP != 0) return false;
    return (long long)c.B * c.Hkv * nqb <= 0x7fffffffLL;
}

template <class Geo>
static hipError_t fa_window_launch(const Int8Workspace& w, const float* Qf, float* O, const MaskedCall& c, int window, hipStream_t stream,
                                   Geo geo) {
    const int nqb = masked_nqb(grid_units(geo));
    if (!window_shape_ok(c, window, nqb)) return hipErrorInvalidValue;
    const Window<Geo> wg(geo, window / QMHA_GROUP);
    const dim3 grid(c.B * c.Hkv * nqb), block(kWaves * 64);
    return int8_masked_d(c.D, [&](auto d) {
        hipLaunchKernelGGL((qmha_fa_int8_window_kernel<Geo, decltype(d)::value>), grid, block, 0, stream, Qf, w.Ki, w.Vh, w.sK, w.sV, O,
                           wg, c.lens, c.Hkv, c.d_model, nqb, softmax_scale_log2(c.D));
        return hipGetLastError();
    });
}

template <class Geo>
static hipError_t fa_window_launch(const F16Workspace& w, const float* Qf, float* O, const MaskedCall& c, int window, hipStream_t stream,
                                   Geo geo) {
    const int nqb = masked_nqb(grid_units(geo));
    if (!window_shape_ok(c, window, nqb)) return hipErrorInvalidValue;
    const Window<Geo> wg(geo, window / QMHA_GROUP);
    const dim3 grid(c.B * c.Hkv * nqb), block(kWaves * 64);
    return f16_masked_d(c.D, [&](auto d) {
        hipLaunchKernelGGL((qmha_fa_f16_window_kernel<Geo, decltype(d)::value>), grid, block, 0, stream, Qf, w.Kh, w.Vt, O, wg, c.lens,
                           c.Hkv, c.d_model, nqb, softmax_scale_log2(c.D));
        return hipGetLastError();
    });
}

// The instances of this file, in the order they stand in its code object
#define QMHA_WINDOW_INSTANCE(W, G) \
    template hipError_t fa_window_launch<G>(const W&, const float*, float*, const MaskedCall&, int, hipStream_t, G);
QMHA_WINDOW_INSTANCE(Int8Workspace, Ragged)
QMHA_WINDOW_INSTANCE(F16Workspace, Ragged)
QMHA_WINDOW_INSTANCE(Int8Workspace, Paged)
QMHA_WINDOW_INSTANCE(F16Workspace, Paged)
#undef QMHA_WINDOW_INSTANCE

template <class W>
static hipError_t window_any(const W& w, const float* Qf, float* O, const MaskedCall& c, int window, hipStream_t stream) {
    if (!c.ragged) return hipErrorInvalidValue;
    return masked_geo(c, [&](auto geo) {
        if constexpr (kRaggedGeo<decltype(geo)>) return fa_window_launch(w, Qf, O, c, window, stream, geo);
        else return hipErrorInvalidValue;
    });
}
hipError_t launch_fa_window(const Int8Workspace& w, const float* Qf, float* O, const MaskedCall& c, int window, hipStream_t stream) {
    return window_any(w, Qf, O, c, window, stream);
}
hipError_t launch_fa_window(const F16Workspace& w, const float* Qf, float* O, const MaskedCall& c, int window, hipStream_t stream) {
    return window_any(w, Qf, O, c, window, stream);
}

}  // namespace qmha
