// qmha_fa_packed.hip -- packed batches for the token-granular and paged attends of a K/V cache, for
// gfx950 (MI355X): Q and O are [total, d_model] with no batch axis, and a device array int32 cu[B + 1] gives sequence b
// the rows [cu[b], cu[b + 1]) -- a query count of its own per sequence, read when the kernel runs.  The kernels are the
// cache kernels of qmha_fa_masked.hpp (qmha_fa_{int8,f16}_cache_kernel, whose prologue for a packed sequence is
// packed_seq there) over Packed<Ragged> and Packed<Paged>, instantiated here: a translation unit of its own for the
// reason qmha_fa_split.hip is one.
#include "qmha_fa_masked.hpp"

namespace qmha {

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
        hipLaunchKernelGGL((qmha_fa_int8_cache_kernel<decltype(d)::value, Packed<Geo>>), grid, block, 0, stream, Qf, w.Ki, w.Vh, w.sK, w.sV,
                           O, pg, c.lens, c.Hkv, c.d_model, nqb, softmax_scale_log2(c.D));
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
        hipLaunchKernelGGL((qmha_fa_f16_cache_kernel<decltype(d)::value, Packed<Geo>>), grid, block, 0, stream, Qf, w.Kh, w.Vt, O, pg,
                           c.lens, c.Hkv, c.d_model, nqb, softmax_scale_log2(c.D));
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
