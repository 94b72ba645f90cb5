// qmha_kernels.hpp -- internal (non-ABI) launcher declarations shared by the kernel
// translation units and the C-ABI layer (qmha_api.cpp).
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <type_traits>

namespace qmha {

inline constexpr size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// log2(e): the fused kernels' softmax runs in base 2 (v_exp_f32), scores pre-multiplied by log2(e).
inline constexpr float kLog2e = 1.4426950408889634f;
// the launchers' c_log2 = 1/sqrt(d) * log2(e) (inv_sqrt_d: fa_tc_int8_b.cu:587)
inline float softmax_scale_log2(int D) { return (1.0f / sqrtf((float)D)) * kLog2e; }

// A workspace layout is stated once, as the order in which its carve takes the arrays: with a null base
// the same walk only adds up the size, so *_workspace_bytes and *_carve cannot disagree.
struct Carver {
    char* base;
    size_t used = 0;
    template <class T>
    T* take(size_t bytes) {  // `bytes` already a multiple of 256
        T* p = base ? reinterpret_cast<T*>(base + used) : nullptr;
        used += bytes;
        return p;
    }
};

// Tuning knob for benchmarking kernel geometries: env var "<waves>x<stages>" (e.g. "8x2")
// read once per variable; returns waves*10+stages, or 0 (= built-in default).
int tune_config(const char* env_name);

// ---- INT8 (fa_tc_int8_b) ---------------------------------------------------------------
struct Int8Workspace {
    int8_t* Qi;  // [B*H][N][D]  (test hook only: nullptr in the production carve)
    int8_t* Ki;  // [B*H][N][D]
    _Float16* Vh;  // [B*H][N/32][D][32]  quantised V as f16 integers (f16 operand slot order)
    float* sQ;   // [B*H][N/32]  (per-tensor mode: [B*H], one scale per head slice)
    float* sK;
    float* sV;
    uint32_t* slice_sync;  // per-tensor mode only: [2][3][B*H] slice absmax bits and part arrivals (qmha_pt_quant_kernel)
    size_t bytes;          // of the whole layout (set by the carves)
};
// Production layout: Ki [B*H][N][D], Vh (f16 V^T operand blocks, 2 bytes per element), sK, sV
// [B*H][N/32] (the main kernel quantises Q in registers).  with_q adds Qi and sQ at the end for the
// int32 Q@K^T test hook, whose pre-pass quantises Q too.
inline Int8Workspace int8_carve(void* ws, int B, int N, int H, int D, bool with_q = false) {
    const size_t e = align_up((size_t)B * H * N * D, 256);
    const size_t s = align_up((size_t)B * H * (N / 32) * sizeof(float), 256);  // 32-row quantisation groups
    Carver c{static_cast<char*>(ws)};
    Int8Workspace w{};
    w.Ki = c.take<int8_t>(e);
    w.Vh = c.take<_Float16>(2 * e);
    w.sK = c.take<float>(s);
    w.sV = c.take<float>(s);
    if (with_q) {
        w.Qi = c.take<int8_t>(e);
        w.sQ = c.take<float>(s);
    }
    w.bytes = c.used;
    return w;
}
inline size_t int8_workspace_bytes(int B, int N, int H, int D, bool with_q = false) {
    return int8_carve(nullptr, B, N, H, D, with_q).bytes;
}
// v_mode 0: V to `vout` as int8 in the i8 operand order; 1: as f16 integers (main path)
// first_tensor = 1 skips Q (the main kernels quantise Q themselves); 0 quantises Q, K, V;
// num_tensors (default: all from first_tensor on) limits the roles launched (the standalone op)
hipError_t launch_quant_int8(const float* Q, const float* K, const float* V, const Int8Workspace& w, void* vout,
                             int v_mode, int B, int N, int H, int D, int d_model, hipStream_t stream,
                             int first_tensor = 0, int num_tensors = -1);
// ---- INT8 per-tensor mode (fa_tc_int8_pt) ----------------------------------------------
// layout: Ki, Vh as fa_tc_int8_b, then slice_sync [2][3][B*H] uint32, then sQ, sK, sV [B*H] each
inline size_t pt_slice_sync_bytes(int B, int H) { return align_up((size_t)6 * B * H * sizeof(uint32_t), 256); }
inline Int8Workspace int8_pt_carve(void* ws, int B, int N, int H, int D) {
    const size_t e = align_up((size_t)B * H * N * D, 256);
    const size_t s = align_up((size_t)B * H * sizeof(float), 256);
    Carver c{static_cast<char*>(ws)};
    Int8Workspace w{};
    w.Ki = c.take<int8_t>(e);
    w.Vh = c.take<_Float16>(2 * e);
    w.slice_sync = c.take<uint32_t>(pt_slice_sync_bytes(B, H));
    w.sQ = c.take<float>(s);
    w.sK = c.take<float>(s);
    w.sV = c.take<float>(s);
    w.bytes = c.used;
    return w;
}
inline size_t int8_pt_workspace_bytes(int B, int N, int H, int D) { return int8_pt_carve(nullptr, B, N, H, D).bytes; }
// one pass: K / V quantised with their head-slice scales from registers, sQ (qmha_pt_quant_kernel)
// the per-tensor pre-pass's bounded wait in 100 MHz ticks (default 200000 = 2 ms; 0 forces the
// fallback); returns the previous value
long long set_pt_wait_ticks(long long ticks);
hipError_t launch_quant_int8_pt(const float* Q, const float* K, const float* V, const Int8Workspace& w, int B, int N,
                                int H, int D, int d_model, hipStream_t stream);
// the standalone op's per-tensor layout: X in the K role only (int8 rows, one scale per head slice)
hipError_t launch_quant_int8_pt_rows(const float* X, const Int8Workspace& w, int B, int N, int H, int D, int d_model,
                                     hipStream_t stream);
hipError_t launch_fa_int8_pt_main(const Int8Workspace& w, const float* Qf, float* O, int B, int N, int H, int D,
                                  int d_model, hipStream_t stream);
// Qf: the caller's fp32 Q (the main kernel quantises each Q group into its MFMA operand)
hipError_t launch_fa_int8_main(const Int8Workspace& w, const float* Qf, float* O, int B, int N, int H, int D,
                               int d_model, hipStream_t stream);
hipError_t launch_debug_qk_int32(const Int8Workspace& w, int N, int D, int bh, int32_t* S, hipStream_t stream);
// what the production int8 kernel computed (FL_DUMP instance): S [B*H][N][N] int32 (bias
// removed), Qi [B*H][N][D] (its in-register Q operand), sQ [B*H][N/32]
struct QkDump {
    int32_t* S;
    int8_t* Qi;
    float* sQ;
};
// what a dumping instance of the per-block kernels stores beside QkDump, per tile a wave computes (the P stage;
// all null: nothing): m [B*H][Nq][Gk] the row's running max after the tile (log2 units); sP [B*H][Gq][Gk] the
// tile's P scale (without the 2^24 of the f16-subnormal packing); Pi [B*H][Nq][Nk] the quantised P entry read back
// from the packed f16 MFMA operand; T [B*H][Gk][Nq][D] the tile's P@V accumulator as int32 (INT32_MIN where the
// accumulator was not an integer); l [B*H][Nq] the joined, un-anchored row sum the epilogue divides by.
// Gq = Nq / 32, Gk = Nk / 32.  The shipped kernels' arguments are not touched: the non-causal kernels' dumping
// instances read it from a device variable of their translation unit, the masked kernel's from their geometry.
struct PDump {
    float* m;
    float* sP;
    int8_t* Pi;
    int32_t* T;
    float* l;
};
hipError_t launch_fa_int8_dump(const Int8Workspace& w, const float* Qf, float* O, int B, int N, int H, int D,
                               int d_model, QkDump dbg, hipStream_t stream);
// The dumping twin of the kernel launch_fa_int8_main (Nq == Nk, not causal; launch_fa_masked's is declared with it
// below) would launch for this shape, N = 32 included; every buffer of dbg and pd is written.  On the null stream, for
// the blocking debug hook: the non-causal twins' device variable is set before the launch and cleared after it with
// blocking copies.
hipError_t launch_fa_int8_pstage_dump(const Int8Workspace& w, const float* Qf, float* O, int B, int N, int H, int D,
                                      int d_model, QkDump dbg, PDump pd);
hipError_t launch_fa_int8_pt_dump(const Int8Workspace& w, const float* Qf, float* O, int B, int N, int H, int D,
                                  int d_model, QkDump dbg, hipStream_t stream);

// ---- FP16 (fa_tc_v1a) ------------------------------------------------------------------
struct F16Workspace {  // no Q: the main kernel converts Q in registers
    _Float16* Kh;  // [B*H][N][D]
    _Float16* Vt;  // [B*H][N/32][D][32]  (f16 operand slot order)
    size_t bytes;  // of the whole layout (set by the carve)
};
inline F16Workspace f16_carve(void* ws, int B, int N, int H, int D) {
    const size_t e = align_up((size_t)B * H * N * D * 2, 256);
    Carver c{static_cast<char*>(ws)};
    F16Workspace w{};
    w.Kh = c.take<_Float16>(e);
    w.Vt = c.take<_Float16>(e);
    w.bytes = c.used;
    return w;
}
inline size_t f16_workspace_bytes(int B, int N, int H, int D) { return f16_carve(nullptr, B, N, H, D).bytes; }
hipError_t launch_convert_f16(const float* Q, const float* K, const float* V, const F16Workspace& w, int B, int N,
                              int H, int D, int d_model, hipStream_t stream);
hipError_t launch_fa_f16_main(const F16Workspace& w, const float* Qf, float* O, int B, int N, int H, int D, int d_model,
                              hipStream_t stream);

// ---- the built head sizes of the masked and cache kernels: f(std::integral_constant<int, D>) --------
template <class F>
hipError_t int8_masked_d(int D, F&& f) {
    switch (D) {
        case 32: return f(std::integral_constant<int, 32>{});
        case 64: return f(std::integral_constant<int, 64>{});
        case 128: return f(std::integral_constant<int, 128>{});
        default: return hipErrorInvalidValue;
    }
}
template <class F>
hipError_t f16_masked_d(int D, F&& f) {
    switch (D) {
        case 64: return f(std::integral_constant<int, 64>{});
        case 128: return f(std::integral_constant<int, 128>{});
        default: return hipErrorInvalidValue;
    }
}

// ---- masked main kernels (qmha_fa_masked.hip) ---------------------
// One launch of the masked templates.  Q / O: [B, Nq, d_model = H * D].  w: the variant's carve over K / V of Hkv heads
// and Nk rows -- the workspace of the non-causal paths, whose pre-pass ran unchanged with N = Nk, H = Hkv and
// d_model = Hkv * D; Hkv < H (H % Hkv == 0) is grouped-query attention.  Nq, Nk multiples of 32.  The modes:
//   a call of its own (len < 0, lens null): all Nk rows.  causal: bottom-right aligned, row r attends keys
//     j <= r + Nk - Nq (Nk >= Nq).  Hkv == H: SquareCausal when causal and Nq == Nk, else Rect; Hkv < H: Grouped.
//   a K/V cache (len >= 0): Nk = cap, and `len` of the cap rows per slice are valid (len % 32 == 0).  causal: over the
//     first len rows (j <= r + len - Nq, Nq <= len <= cap), diag_off = (len - Nq) / 32, so no tile at or beyond
//     len / 32 is staged or computed; not causal: every row attends all cap rows, which needs len == cap.  Always Rect
//     (or Grouped over it), also at Nq == len.
//   per-sequence lengths (lens: DEVICE int32[B], read by the kernel; the grid follows the host arguments only): the
//     varlen kernels, Hkv == H included.  Sequence b computes what the cache mode computes at len = lens[b] -- without
//     the mask over rows [0, lens[b]), whatever cap is --; lens[b] % 32 != 0, > cap, < Nq (causal) or < 32 (not): its O
//     rows are zeros and none of its K/V is read.
//   token-granular lengths (ragged, with lens and causal): the ragged kernels.  Any 1 <= Nq <= Nk; sequence
//     b, Nq <= lens[b] <= Nk, computes rows [s, s + Nq), s = (lens[b] - Nq) mod 32, of the per-sequence-length mode on a
//     zero block of ceil32(s + Nq) rows holding Q there, at ceil32(lens[b]); any other lens[b]: its Nq rows of O are zeros.
//   a paged cache (ragged, with a table): the paged kernels.  w is the carve of a pool of num_pages pages
//     (B := num_pages, N := page_rows, H := Hkv), Nk the logical capacity max_pages * page_rows, and row r of sequence b lies
//     in page table[b][r / page_rows] (DEVICE int32 [B][max_pages], read by the kernel) at row r % page_rows.  A valid
//     sequence computes the bits of the token-granular mode on a contiguous cache holding its rows; lens[b] outside
//     [Nq, Nk], or an entry of a page it uses outside [0, num_pages): its Nq rows of O are zeros, none of its K/V is read.
// B * Hkv K/V slices per grid.  int8: d in {32, 64, 128}; fp16: d in {64, 128} (qmha_api.cpp's variant table).  A shape
// or head count outside the above, d_model != H * D, an unbuilt d: hipErrorInvalidValue, nothing launched.
// The block table of a paged cache (null table: a contiguous cache); page_rows % 64 == 0
struct PageTable {
    const int32_t* table = nullptr;
    int page_rows = 0, max_pages = 0, num_pages = 0;
};
struct MaskedCall {
    int B, Nq, Nk, H, Hkv, D, d_model;
    bool causal;
    int len;
    const int32_t* lens;
    bool ragged = false;  // lens at token granularity (the ragged kernels): any 1 <= Nq <= Nk, causal only
    PageTable pages = {};  // with ragged and a table: a paged cache (the paged kernels), Nk = max_pages * page_rows
};
hipError_t launch_fa_masked(const Int8Workspace& w, const float* Qf, float* O, const MaskedCall& c, hipStream_t stream);
hipError_t launch_fa_masked(const F16Workspace& w, const float* Qf, float* O, const MaskedCall& c, hipStream_t stream);
// The dumping twin of the instance launch_fa_masked launches for a call of its own with Hkv == H; no other mode has one
hipError_t launch_fa_int8_masked_pstage_dump(const Int8Workspace& w, const float* Qf, float* O, const MaskedCall& c, QkDump dbg,
                                             PDump pd);

// ---- split-KV over a cache's token-granular and paged calls (qmha_fa_split.hip) -----------
// The caller's scratch of a split call, each array on a multiple of 256 bytes: per sequence b, chunk c < NC =
// ceil(Nk / chunk_rows), real query row r < Nq and query head k < H the chunk's normalised output Oc [B][NC][Nq][H * D],
// its row sum l and its running maximum m (log2 units), both [B][NC][Nq][H], all fp32.  Only the entries of chunks a row
// reaches (c * chunk_rows / 32 <= its group's last tile) are written, and only those are read.
struct SplitScratch {
    float *Oc, *m, *l;
    size_t bytes;  // of the whole layout
};
inline SplitScratch split_carve(void* p, int B, int NC, int Nq, int H, int D) {
    const size_t rows = (size_t)B * NC * Nq;
    Carver c{static_cast<char*>(p)};
    SplitScratch s{};
    s.Oc = c.take<float>(align_up(rows * H * D * sizeof(float), 256));
    s.m = c.take<float>(align_up(rows * H * sizeof(float), 256));
    s.l = c.take<float>(align_up(rows * H * sizeof(float), 256));
    s.bytes = c.used;
    return s;
}
// c: a token-granular call (ragged, with lens; a table: paged) as launch_fa_masked takes it.  Two launches on `stream`:
// the partial kernels, a workgroup per (K/V slice, unit block, chunk of chunk_rows key rows), fill `scratch`
// (split_carve(..).bytes bytes, 256-byte aligned); the combine kernel writes O.  chunk_rows: a multiple of 64 in [64, Nk].
hipError_t launch_fa_split(const Int8Workspace& w, const float* Qf, float* O, const MaskedCall& c, int chunk_rows, void* scratch,
                           hipStream_t stream);
hipError_t launch_fa_split(const F16Workspace& w, const float* Qf, float* O, const MaskedCall& c, int chunk_rows, void* scratch,
                           hipStream_t stream);

// ---- a sliding window over a cache's token-granular and paged calls (qmha_fa_window.hip) -----------
// c: a token-granular call (ragged, with lens; a table: paged) as launch_fa_masked takes it.  window: a multiple of 32,
// >= 32, no upper limit.  With L = lens[b], real row i of the Nq rows attends the cache rows j with
// i + L - Nq - window < j <= i + L - Nq: the last min(window, i + L - Nq + 1) of those launch_fa_masked gives it; a window
// that reaches row 0 of every sequence gives launch_fa_masked's bits.  A paged call loads only the table columns whose
// pages hold rows [64 * (first / 2), L), first = max(0, (ceil32(L) - ceil32(s + Nq) - window) / 32) the first tile of the
// first query group; an entry outside the pool among them, or lens[b] outside [Nq, Nk]: the sequence's rows of O are zeros.
hipError_t launch_fa_window(const Int8Workspace& w, const float* Qf, float* O, const MaskedCall& c, int window, hipStream_t stream);
hipError_t launch_fa_window(const F16Workspace& w, const float* Qf, float* O, const MaskedCall& c, int window, hipStream_t stream);

// ---- K/V cache append (qmha_prepass.hip) ----------------------------------------
// w: the variant's carve of H heads at N = cap, in caller-owned memory.  The pre-pass of the n new rows K, V
// [B, n, d_model = H * D] into rows [len, len + n) of every slice, byte for byte what the pre-pass of a whole call writes
// there; n, cap, len multiples of 32, len + n <= cap.  pos non-null (DEVICE int32[B], read by the kernel; len ignored):
// sequence b's rows go to [pos[b], pos[b] + n); pos[b] < 0, pos[b] % 32 != 0 or pos[b] + n > cap: that sequence writes
// nothing.  Bad host arguments: hipErrorInvalidValue.
template <class W>  // Int8Workspace or F16Workspace, as for the two below
hipError_t launch_kv_append(const float* K, const float* V, const W& w, int B, int n, int cap, int len, const int32_t* pos, int H, int D,
                            int d_model, hipStream_t stream);

// Token-granular append: any 1 <= n <= cap rows per sequence at any row pos[b] (DEVICE int32[B], non-null);
// every 32-row group that rows [pos[b], pos[b] + n) touch is written as the append kernels write that group's rows so
// far, zero-padded.  tail: the int8 cache's raw fp32 rows of each sequence's open group, [2][B][32][d_model] (K, then V),
// read for the rows ahead of pos[b] in its group and rewritten while the last group stays open; fp16 has none (ignored).
// pos[b] < 0 or pos[b] + n > cap: that sequence writes nothing.  Bad host arguments: hipErrorInvalidValue.
// pt with a table: w is the carve of a pool of pages, cap = max_pages * page_rows, and group g of sequence
// b goes to group g % (page_rows / 32) of page table[b][g / (page_rows / 32)]; an entry of a touched page outside
// [0, num_pages) is an invalid pos[b].  The tail stays per sequence.
inline size_t kv_tail_bytes(int B, int H, int D) { return align_up((size_t)2 * B * 32 * H * D * sizeof(float), 256); }
template <class W>
hipError_t launch_kv_tokens(const float* K, const float* V, const W& w, float* tail, int B, int n, int cap, const int32_t* pos, int H, int D,
                            int d_model, hipStream_t stream, const PageTable& pt = {});

// ---- packed batches (qmha_fa_packed.hip, qmha_prepass.hip) ---------------------------------
// The token-granular / paged attend and append on operands without a batch axis: Q, O [total, d_model], K, V
// [rows, H * D], and cu (DEVICE int32 [B + 1], read by the kernels) gives sequence b the rows [cu[b], cu[b + 1]).
// Attend: c is a token-granular call as launch_fa_masked takes it (ragged, with lens; a table: paged) whose Nq is the
// bound max_nq the grid is sized for, 1 <= max_nq <= min(total, Nk).  A sequence with 1 <= nq_b <= max_nq rows and
// nq_b <= lens[b] <= Nk gets the bits of that call at Nq = nq_b; nq_b == 0: it sits out; a range outside
// 0 <= cu[b] <= cu[b + 1] <= total: nothing of it is read or written; any other: its rows of O are zeros.
// Append: launch_kv_tokens with n_b = cu[b + 1] - cu[b] rows for sequence b, 1 <= max_n <= min(rows, cap) the bound the
// items are sized for; n_b == 0, n_b > max_n, a bad range, pos[b] < 0 or pos[b] + n_b > cap (or a touched table entry
// outside the pool): that sequence writes nothing, the tail included.  Bad host arguments: hipErrorInvalidValue.
hipError_t launch_fa_packed(const Int8Workspace& w, const float* Qf, float* O, const MaskedCall& c, const int32_t* cu, int total,
                            hipStream_t stream);
hipError_t launch_fa_packed(const F16Workspace& w, const float* Qf, float* O, const MaskedCall& c, const int32_t* cu, int total,
                            hipStream_t stream);
template <class W>
hipError_t launch_kv_packed(const float* K, const float* V, const W& w, float* tail, int B, int rows, int max_n, int cap, const int32_t* cu,
                            const int32_t* pos, int H, int D, int d_model, hipStream_t stream, const PageTable& pt = {});

// ---- FP32 (fa: scalar VALU kernel; fa_mfma: the same contract on v_mfma_f32_32x32x2_f32) -----
hipError_t launch_fa_f32(const float* Q, const float* K, const float* V, float* O, int B, int N, int H, int D,
                         int d_model, bool mfma, hipStream_t stream);

// ---- unfused 3-kernel baseline (unfused.cu) --------------------------------------------
size_t unfused_workspace_bytes(int B, int N, int H, int D);
hipError_t launch_unfused(const float* Q, const float* K, const float* V, float* O, void* ws, int B, int N, int H,
                          int D, int d_model, hipStream_t stream);

}  // namespace qmha
