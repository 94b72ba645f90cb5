// qmha_fp8.hpp -- what the attend kernels of an e4m3 K/V cache share (qmha_fa_fp8.hip, qmha_fp8_decode.hip):
// the MFMA operand types and the contract's conversion of fp32 values into an operand.
#pragma once

#include "qmha_common.hpp"

namespace qmha {

typedef long fp8x8;  // eight e4m3 bytes: one MFMA operand
typedef long v2l __attribute__((ext_vector_type(2)));  // a ds_read_b128: two operands

// eight floats, already scaled and clamped, as one operand (RNE; two values per v_cvt_pk_fp8_f32)
__device__ __forceinline__ fp8x8 fp8_pack8(const float (&x)[8]) {
    int lo = 0, hi = 0;
    lo = __builtin_amdgcn_cvt_pk_fp8_f32(x[0], x[1], lo, false);
    lo = __builtin_amdgcn_cvt_pk_fp8_f32(x[2], x[3], lo, true);
    hi = __builtin_amdgcn_cvt_pk_fp8_f32(x[4], x[5], hi, false);
    hi = __builtin_amdgcn_cvt_pk_fp8_f32(x[6], x[7], hi, true);
    return (fp8x8)(((unsigned long)(unsigned)hi << 32) | (unsigned)lo);
}
// the contract's element: clamp in fp32 ahead of the convert, so its overflow behaviour is never asked for
__device__ __forceinline__ float fp8_prep(float x, float scale) { return fminf(fmaxf(x / scale, -448.0f), 448.0f); }

}  // namespace qmha
