// qmha_kv_fp8.hip -- the appends of an e4m3 K/V cache (fa_tc_fp8), in a translation unit of their own: they
// read the caller's K / V, so they keep IEEE semantics as qmha_prepass.hip does, and no shipped kernel's bytes move.
// One template over two policies, which come first in its argument list, D after them:
//   Row   the first cache row a sequence writes: the host's len (LenRow, qmha_kv_cache_append), pos[b] read on the device
//         at a multiple of 32 (PosRow<true>, _append_at) or at any row (PosRow<false>, _append_tokens / _append_paged)
//   Dst   where group g of a K/V slice lies: `cap` rows a slice (SliceRows) or the pages of a pool behind a block table on
//         the device (PoolRows)
// They are the policies of the fp16 appends (HostRow, PlacedRow, UniformRows x ContiguousRows / PagedTable) restated for a
// cache without a tail; those live in qmha_prepass.hip, whose text is part of its kernels' bytes.
// A cached element is e4m3_rne(clamp(x / scale, -448, 448)), the clamp in fp32 ahead of v_cvt_pk_fp8_f32.  One wave per
// (tensor, K/V slice, touched 32-row group): rows [p, p + n) of a sequence touch groups p / 32 .. (p + n - 1) / 32, at
// most (n + 30) / 32 + 1.  The zero-padding rules are the fp16 appends': a group the call opens (p at or before its first
// row) is written whole, zeros behind the new rows; a group earlier rows opened gets the new rows only and relies on the
// rows behind them being zero.
//   K   e4m3 rows [slice][cap][D]: a lane converts four columns of a row into one dword.
//   V   the group's V^T block (fp8_vt_offset): four consecutive key rows of one d are four consecutive bytes, and a lane
//       owns that whole dword -- in a group that stays open it loads the dword, keeps the bytes of the rows ahead of p and
//       stores it back, so no two lanes ever share a dword and no byte store races.
#include "qmha_common.hpp"
#include "qmha_kernels.hpp"

namespace qmha {

struct LenRow {
    int len;
    __device__ __forceinline__ int first(int) const { return len; }
};
template <bool ALIGNED>
struct PosRow {
    const int32_t* __restrict__ pos;  // DEVICE int32 [B]
    __device__ __forceinline__ int first(int b) const {
        const int p = __builtin_amdgcn_readfirstlane(pos[b]);
        return ALIGNED && (p & (QMHA_GROUP - 1)) != 0 ? -1 : p;  // two's complement: of a negative value too
    }
};
struct SliceRows {
    int cap;
    __device__ __forceinline__ int capacity() const { return cap; }
    __device__ __forceinline__ bool ok(int, int, int) const { return true; }
    __device__ __forceinline__ size_t group(int b, int kh, int H, int g) const { return ((size_t)b * H + kh) * (cap / QMHA_GROUP) + g; }
};
struct PoolRows {
    const int32_t* table;  // DEVICE int32 [B][max_pages]
    int PG, max_pages, num_pages;
    __device__ __forceinline__ int capacity() const { return max_pages * PG * QMHA_GROUP; }
    // every entry of the pages that groups g0 .. g1 of sequence b touch lies in the pool (lanes take the columns; the
    // same verdict in every wave of the sequence, which all scan the same entries)
    __device__ __forceinline__ bool ok(int b, int g0, int g1) const {
        const int c0 = (unsigned)g0 / (unsigned)PG, c1 = (unsigned)g1 / (unsigned)PG;  // <= max_pages - 1: p + n <= capacity
        bool bad = false;
        for (int c = c0 + (threadIdx.x & 63); c <= c1; c += 64) bad |= (unsigned)table[(size_t)b * max_pages + c] >= (unsigned)num_pages;
        return __builtin_amdgcn_ballot_w64(bad) == 0;
    }
    __device__ __forceinline__ size_t group(int b, int kh, int H, int g) const {
        const unsigned c = (unsigned)g / (unsigned)PG;
        // valid (ok above); clamped all the same, so that no table content leaves the pool
        const unsigned page = min((unsigned)__builtin_amdgcn_readfirstlane(table[(size_t)b * max_pages + c]), (unsigned)(num_pages - 1));
        return ((size_t)page * H + kh) * PG + ((unsigned)g - c * (unsigned)PG);
    }
};

// four elements as one dword of e4m3 bytes
__device__ __forceinline__ uint32_t fp8_pack4(const float (&x)[4], float scale) {
    float y[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) y[c] = fminf(fmaxf(x[c] / scale, -448.0f), 448.0f);
    int w = 0;
    w = __builtin_amdgcn_cvt_pk_fp8_f32(y[0], y[1], w, false);
    w = __builtin_amdgcn_cvt_pk_fp8_f32(y[2], y[3], w, true);
    return (uint32_t)w;
}

template <class Row, class Dst, int D>
__global__ __launch_bounds__(256) void qmha_fp8_kv_kernel(const float* __restrict__ K, const float* __restrict__ V, uint8_t* __restrict__ K8,
                                                          uint8_t* __restrict__ Vt8, int n, Row row, Dst dst, int H, int d_model, int maxg,
                                                          int total, float k_scale, float v_scale) {
    const int lane = threadIdx.x & 63;
    const int item = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));  // (K/V slice, j)
    if (item >= total) return;  // per wave; no workgroup barrier follows
    const int bh = item / maxg, j = item % maxg;
    const int b = bh / H, kh = bh % H;
    const int p = row.first(b);
    if (p < 0 || p > dst.capacity() - n) return;  // an invalid row: the sequence writes nothing
    const int g0 = p / QMHA_GROUP, g1 = (p + n - 1) / QMHA_GROUP, g = g0 + j;
    if (g > g1 || !dst.ok(b, g0, g1)) return;
    const size_t gi = dst.group(b, kh, H, g);
    const int lo = p - g * QMHA_GROUP, hi = lo + n;  // the new rows of this group: lo <= r < hi
    const bool opens = lo <= 0;                      // else rows [0, lo) are earlier appends' and stay
    const float* src = (blockIdx.y ? V : K) + ((ptrdiff_t)b * n - lo) * d_model + (ptrdiff_t)kh * D;  // row r of the group: src + r * d_model
    if (blockIdx.y == 0) {
        constexpr int C4 = D / 4, RPI = 64 / C4;
        const int ri = lane / C4, ci = lane % C4;
        uint8_t* out = K8 + gi * (size_t)(QMHA_GROUP * D) + 4 * ci;
#pragma unroll 4
        for (int r = ri; r < QMHA_GROUP; r += RPI) {
            if (r < lo || (r >= hi && !opens)) continue;
            float x[4] = {};
            if (r < hi) {
                const v4f v = __builtin_nontemporal_load(reinterpret_cast<const v4f*>(src + (ptrdiff_t)r * d_model + 4 * ci));
#pragma unroll
                for (int c = 0; c < 4; ++c) x[c] = v[c];
            }
            *reinterpret_cast<uint32_t*>(out + (size_t)r * D) = fp8_pack4(x, k_scale);
        }
        return;
    }
    uint8_t* blk = Vt8 + gi * (size_t)(QMHA_GROUP * D);
#pragma unroll 2
    for (int e = lane; e < D * 8; e += 64) {  // dword (d, a): key rows 4 a .. 4 a + 3 of V^T row d
        const int d = e % D, r0 = 4 * (e / D);
        if (r0 + 4 <= lo || (r0 >= hi && !opens)) continue;
        float x[4] = {};
#pragma unroll
        for (int c = 0; c < 4; ++c)
            if (r0 + c >= lo && r0 + c < hi) x[c] = src[(ptrdiff_t)(r0 + c) * d_model + d];
        uint32_t w = fp8_pack4(x, v_scale);
        uint32_t* out = reinterpret_cast<uint32_t*>(blk + fp8_vt_offset(d, r0));
        if (r0 < lo) {  // lo > 0: the group stays open, bytes of rows r0 .. lo - 1 are kept
            const uint32_t keep = (1u << (8 * (lo - r0))) - 1u;
            w = (w & ~keep) | (*out & keep);
        }
        *out = w;
    }
}

template <class Row, class Dst>
static hipError_t kv_fp8_launch(const float* K, const float* V, const Fp8Workspace& w, int B, int n, Row row, Dst dst, int maxg, int H, int D,
                                int d_model, hipStream_t stream) {
    if ((long long)B * H * maxg > 0x7fffffffLL) return hipErrorInvalidValue;
    const int total = B * H * maxg;
    const dim3 grid((total + 3) / 4, 2);
    return fp8_cache_d(D, [&](auto d) {
        hipLaunchKernelGGL((qmha_fp8_kv_kernel<Row, Dst, decltype(d)::value>), grid, dim3(256), 0, stream, K, V, w.K8, w.Vt8, n, row, dst, H,
                           d_model, maxg, total, w.k_scale, w.v_scale);
        return hipGetLastError();
    });
}

// whole 32-row groups behind the host's len, or at pos[b] (a multiple of 32, read on the device)
hipError_t launch_kv_append(const float* K, const float* V, const Fp8Workspace& w, int B, int n, int cap, int len, const int32_t* pos, int H,
                            int D, int d_model, hipStream_t stream) {
    if (pos) len = 0;
    if (B < 1 || H < 1 || n < QMHA_GROUP || n % QMHA_GROUP != 0 || cap % QMHA_GROUP != 0 || len < 0 || len % QMHA_GROUP != 0 ||
        (long long)len + n > cap)
        return hipErrorInvalidValue;
    if (pos) return kv_fp8_launch(K, V, w, B, n, PosRow<true>{pos}, SliceRows{cap}, n / QMHA_GROUP, H, D, d_model, stream);
    return kv_fp8_launch(K, V, w, B, n, LenRow{len}, SliceRows{cap}, n / QMHA_GROUP, H, D, d_model, stream);
}

// any 1 <= n <= cap rows at any row pos[b]; pt with a table: the pool's pages
hipError_t launch_kv_tokens(const float* K, const float* V, const Fp8Workspace& w, float*, int B, int n, int cap, const int32_t* pos, int H, int D,
                            int d_model, hipStream_t stream, const PageTable& pt) {
    if (B < 1 || H < 1 || !pos || n < 1 || cap < QMHA_GROUP || cap % QMHA_GROUP != 0 || n > cap) return hipErrorInvalidValue;
    const int maxg = (n + QMHA_GROUP - 2) / QMHA_GROUP + 1;  // the groups n rows can touch
    if (!pt.table) return kv_fp8_launch(K, V, w, B, n, PosRow<false>{pos}, SliceRows{cap}, maxg, H, D, d_model, stream);
    if (pt.page_rows < 2 * QMHA_GROUP || pt.page_rows % (2 * QMHA_GROUP) != 0 || pt.max_pages < 1 || pt.num_pages < 1 ||
        (long long)pt.max_pages * pt.page_rows != cap)
        return hipErrorInvalidValue;
    return kv_fp8_launch(K, V, w, B, n, PosRow<false>{pos}, PoolRows{pt.table, pt.page_rows / QMHA_GROUP, pt.max_pages, pt.num_pages}, maxg, H, D,
                         d_model, stream);
}

}  // namespace qmha
