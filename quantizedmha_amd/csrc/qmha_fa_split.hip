// qmha_fa_split.hip -- split-KV for the token-granular and paged attends of a K/V cache, for gfx950
// (MI355X): the key sweep of a decode step cut into chunks of whole stages, a workgroup per (K/V slice, unit block,
// chunk), and a combine pass.  The partial kernels are the bodies of qmha_fa_masked.hip's kernels once more
// (qmha_fa_masked_{int8,f16}.inc), over Split<Ragged> and Split<Paged>; the geometries, the stager and masked_geo are
// the shared header's.
#include "qmha_fa_masked.hpp"

namespace qmha {

// ---------------------------------------------------------------------------------------
// Split-KV (Split, qmha_fa_masked.hpp): the ragged / paged prologue over the same bodies, a workgroup per
// (K/V slice, unit block, chunk); one template per precision over Base = Ragged or Paged.  A template of its own beside
// the cache kernels: it has no O argument (adding one would move every kernarg offset).  The partial kernels write the
// scratch only; an invalid sequence (its length, or a used table entry outside the pool) leaves at once --
// workgroup-uniform, before the body's first barrier or DMA issue -- and the combine kernel writes its zeros.  Two plain
// launches on one stream: no atomics, no flags, no waiting on a workgroup.
// The launch bounds are the ragged siblings', but for int8 d = 32: at the siblings' seven waves per SIMD (72 VGPRs) the
// paged instance spilled 12 bytes; with six it needs no scratch.
// ---------------------------------------------------------------------------------------
template <int D, class Base>
__global__ __launch_bounds__(kWaves * 64, D > 64 ? 2 : D > 32 ? 4 : 6) void qmha_fa_int8_split_kernel(
    const float* __restrict__ Qf, const int8_t* __restrict__ Ki, const _Float16* __restrict__ Vh,
    const float* __restrict__ sK, const float* __restrict__ sV, Split<Base> any, const int32_t* __restrict__ lens, int H,
    int d_model, int nqb, float c_log2) {
    using Geo = Split<Base>;
    float* const O = nullptr;  // the body's stores go to out_base(geo, O): the scratch
    int bh_, qb_, c_;
    split_wg(nqb, any.NC, bh_, qb_, c_);  // the body forms the same triple again
    const int L = lens[bh_ / H];
    if (!any.valid(L)) return;
    if constexpr (kPagedGeo<Base>) {
        if (!any.used_pages_ok(bh_ / H, L)) return;
    }
    const Geo geo = any.of(L, c_);
#include "qmha_fa_masked_int8.inc"
}

template <int D, class Base>
__global__ __launch_bounds__(kWaves * 64, D > 64 ? 2 : 4) void qmha_fa_f16_split_kernel(
    const float* __restrict__ Qf, const _Float16* __restrict__ Kh, const _Float16* __restrict__ Vt, Split<Base> any,
    const int32_t* __restrict__ lens, int H, int d_model, int nqb, float c_log2) {
    using Geo = Split<Base>;
    float* const O = nullptr;  // the body's stores go to out_base(geo, O): the scratch
    int bh_, qb_, c_;
    split_wg(nqb, any.NC, bh_, qb_, c_);  // the body forms the same triple again
    const int L = lens[bh_ / H];
    if (!any.valid(L)) return;
    if constexpr (kPagedGeo<Base>) {
        if (!any.used_pages_ok(bh_ / H, L)) return;
    }
    const Geo geo = any.of(L, c_);
#include "qmha_fa_masked_f16.inc"
}

// The combine pass: a thread per 16 bytes of a real row of O.  Row r of sequence b, head k reads the chunks
// c = 0 ... last(qg) / C of its query group -- the ones the partial kernels wrote for it, and nothing else of the
// scratch --, in ascending order, in fp32:  M = max m_c,  a_c = l_c 2^(m_c - M),  Ltot = sum a_c,
// O = Ltot > thr ? (sum a_c Oc_c) / Ltot : 0.  An invalid sequence: positive zeros, no scratch read.  `any` is
// Split<Paged> for both kinds of cache; table null: a contiguous one, no entry is looked at.
__global__ __launch_bounds__(256) void qmha_split_combine_kernel(float* __restrict__ O, Split<Paged> any,
                                                                 const int32_t* __restrict__ lens, int h, int D, float thr) {
    const int W4 = h * D / 4;  // 16-byte pieces of a row
    const unsigned per = ((unsigned)any.Nq * (unsigned)W4 + 255u) / 256u;  // blocks of a sequence
    const int b = (int)(blockIdx.x / per);
    const int L = lens[b];
    bool valid = any.valid(L);
    if (valid && any.table) valid = any.used_pages_ok(b, L);  // block-uniform: every lane takes part in the ballot
    const int i = (int)(blockIdx.x % per) * 256 + threadIdx.x;
    if (i >= any.Nq * W4) return;
    const int r = i / W4, w = i % W4, k = w / (D / 4);
    float* o = O + ((size_t)b * any.Nq + r) * ((size_t)h * D) + 4 * w;
    if (!valid) {
        *reinterpret_cast<v4f*>(o) = v4f{};
        return;
    }
    const Split<Paged> geo = any.of(L, 0);
    const int n = geo.last((geo.s + r) / QMHA_GROUP) / geo.C + 1;  // <= NC: last(qg) <= Gk - 1
    const size_t step = (size_t)geo.Nq * h, at = ((size_t)b * geo.NC * geo.Nq + r) * h + k;  // chunk c: at + c step
    float M = geo.pm[at];
    for (int c = 1; c < n; ++c) M = fmaxf(M, geo.pm[at + c * step]);
    float Ltot = 0.0f;
    v4f acc = v4f{};
    for (int c = 0; c < n; ++c) {
        const float a = geo.pl[at + c * step] * __builtin_amdgcn_exp2f(geo.pm[at + c * step] - M);
        const v4f oc = *reinterpret_cast<const v4f*>(geo.Oc + (((size_t)b * geo.NC + c) * geo.Nq + r) * ((size_t)h * D) + 4 * w);
        Ltot += a;
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] = fmaf(a, oc[e], acc[e]);
    }
    v4f out;
#pragma unroll
    for (int e = 0; e < 4; ++e) out[e] = Ltot > thr ? acc[e] / Ltot : 0.0f;
    *reinterpret_cast<v4f*>(o) = out;
}

static hipError_t launch_split_combine(float* O, const Split<Paged>& sg, const MaskedCall& c, float thr, hipStream_t stream) {
    const dim3 grid((unsigned)(((size_t)c.Nq * c.d_model / 4 + 255) / 256 * c.B)), block(256);  // split_shape_ok: it fits
    hipLaunchKernelGGL(qmha_split_combine_kernel, grid, block, 0, stream, O, sg, c.lens, c.H, c.D, thr);
    return hipGetLastError();
}
static Paged as_paged(const Ragged& r) { return Paged(r, nullptr, 2 * QMHA_GROUP, 1, 1); }  // the combine's argument: no table
static Paged as_paged(const Paged& p) { return p; }

// The chunks of a call, checked: chunk_rows a multiple of 64 in [64, Nk]; the grid fits
static bool split_shape_ok(const MaskedCall& c, int chunk_rows, long long wgs_per_chunk) {
    if (chunk_rows < 2 * QMHA_GROUP || chunk_rows % (2 * QMHA_GROUP) != 0 || chunk_rows > c.Nk) return false;
    if (((long long)c.Nq * c.d_model / 4 + 255) / 256 * c.B > 0x7fffffffLL) return false;  // the combine's grid
    return wgs_per_chunk * ((c.Nk + chunk_rows - 1) / chunk_rows) <= 0x7fffffffLL;
}

template <class Geo>
static hipError_t fa_split_launch(const Int8Workspace& w, const float* Qf, float* O, const MaskedCall& c, int chunk_rows,
                                  void* scratch, hipStream_t stream, Geo geo) {
    const int nqb = masked_nqb(grid_units(geo));
    if (!scratch || !split_shape_ok(c, chunk_rows, (long long)c.B * c.Hkv * nqb)) return hipErrorInvalidValue;
    const int NC = (c.Nk + chunk_rows - 1) / chunk_rows;
    const SplitScratch s = split_carve(scratch, c.B, NC, c.Nq, c.H, c.D);
    const Split<Geo> sg(geo, s, chunk_rows / QMHA_GROUP, NC);
    const dim3 grid(c.B * c.Hkv * nqb * NC), block(kWaves * 64);
    const hipError_t e = int8_masked_d(c.D, [&](auto d) {
        hipLaunchKernelGGL((qmha_fa_int8_split_kernel<decltype(d)::value, Geo>), grid, block, 0, stream, Qf, w.Ki, w.Vh, w.sK, w.sV, sg,
                           c.lens, c.Hkv, c.d_model, nqb, softmax_scale_log2(c.D));
        return hipGetLastError();
    });
    if (e != hipSuccess) return e;
    return launch_split_combine(O, Split<Paged>(as_paged(geo), s, sg.C, NC), c, 1e-20f, stream);  // fa_tc_int8_b.cu:540-578
}

template <class Geo>
static hipError_t fa_split_launch(const F16Workspace& w, const float* Qf, float* O, const MaskedCall& c, int chunk_rows,
                                  void* scratch, hipStream_t stream, Geo geo) {
    const int nqb = masked_nqb(grid_units(geo));
    if (!scratch || !split_shape_ok(c, chunk_rows, (long long)c.B * c.Hkv * nqb)) return hipErrorInvalidValue;
    const int NC = (c.Nk + chunk_rows - 1) / chunk_rows;
    const SplitScratch s = split_carve(scratch, c.B, NC, c.Nq, c.H, c.D);
    const Split<Geo> sg(geo, s, chunk_rows / QMHA_GROUP, NC);
    const dim3 grid(c.B * c.Hkv * nqb * NC), block(kWaves * 64);
    const hipError_t e = f16_masked_d(c.D, [&](auto d) {
        hipLaunchKernelGGL((qmha_fa_f16_split_kernel<decltype(d)::value, Geo>), grid, block, 0, stream, Qf, w.Kh, w.Vt, sg, c.lens,
                           c.Hkv, c.d_model, nqb, softmax_scale_log2(c.D));
        return hipGetLastError();
    });
    if (e != hipSuccess) return e;
    return launch_split_combine(O, Split<Paged>(as_paged(geo), s, sg.C, NC), c, 1e-10f, stream);  // fa_tc_v1a.cu:384-388
}

// The instances of this file, in the order they stand in its code object
#define QMHA_SPLIT_INSTANCE(W, G) \
    template hipError_t fa_split_launch<G>(const W&, const float*, float*, const MaskedCall&, int, void*, hipStream_t, G);
QMHA_SPLIT_INSTANCE(Int8Workspace, Ragged)
QMHA_SPLIT_INSTANCE(F16Workspace, Ragged)
QMHA_SPLIT_INSTANCE(Int8Workspace, Paged)
QMHA_SPLIT_INSTANCE(F16Workspace, Paged)
#undef QMHA_SPLIT_INSTANCE

template <class W>
static hipError_t split_any(const W& w, const float* Qf, float* O, const MaskedCall& c, int chunk_rows, void* scratch, hipStream_t stream) {
    if (!c.ragged) return hipErrorInvalidValue;
    return masked_geo(c, [&](auto geo) {
        if constexpr (kRaggedGeo<decltype(geo)>) return fa_split_launch(w, Qf, O, c, chunk_rows, scratch, stream, geo);
        else return hipErrorInvalidValue;
    });
}
hipError_t launch_fa_split(const Int8Workspace& w, const float* Qf, float* O, const MaskedCall& c, int chunk_rows, void* scratch,
                           hipStream_t stream) {
    return split_any(w, Qf, O, c, chunk_rows, scratch, stream);
}
hipError_t launch_fa_split(const F16Workspace& w, const float* Qf, float* O, const MaskedCall& c, int chunk_rows, void* scratch,
                           hipStream_t stream) {
    return split_any(w, Qf, O, c, chunk_rows, scratch, stream);
}

}  // namespace qmha
