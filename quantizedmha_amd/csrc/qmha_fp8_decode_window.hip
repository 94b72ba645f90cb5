// qmha_fp8_decode_window.hip -- the sliding-window decode call of an e4m3 K/V cache, with attention sinks (fa_tc_fp8,
// DESIGN.md 26) for gfx950 (MI355X), in a translation unit of its own so that every other kernel keeps its bytes.
// qmha_fp8_decode.hip's call sweeps every sequence from key 0 over a grid of ceil(cap / chunk_rows) chunks; a local layer
// (Mistral, Gemma 2/3: windows of 1024 or 4096; gpt-oss: 128 plus a learned sink per head) needs the last `window` keys of
// a row only.  The work split is that kernel's -- the W = G Nq real query rows of a K/V head as the columns of QB MFMA
// blocks, a workgroup per (sequence, K/V head, chunk), wave w = (tile parity tp = w & 1, d-half dh = w >> 1) over two-tile
// LDS-DMA stages, S^T = K Q^T and O^T = V^T P^T on v_mfma_f32_16x16x32_fp8_fp8, the ballot-guarded TRUE running maximum --
// and this is what is its own:
//   first stage  row r sees key j iff e_r - window < j <= e_r, e_r = L - Nq + r.  lo = max(0, L - Nq - window + 1) is the
//                first key any row sees, t0 = 2 (lo / 64) the first tile of the two-tile stage that holds it (in a pool a
//                page's stage), and the sweep is tiles t0 ... (L - 1) / 32: chunk c is tiles t0 + c C ..., PageWalk starts
//                at t0 + c C.  Tiles before t0 are neither staged nor computed, and of a block table only the columns whose
//                pages hold rows [32 t0, L) are read (Paged::used_pages_ok(b, lo, L)).
//   grid         NCw = decode_window_chunks(cap, Nq, window, chunk_rows) chunks per (sequence, K/V head): a sweep covers at
//                most min(cap, Nq + window + 62) rows, whatever L is.
//   left edge    a select to -inf before the maximum, on the tiles whose first key some row does not see
//                (32 t <= L - 1 - window: wave-uniform, as the right edge's test is).
//   empty        with Nq > 1 a late row's left edge can lie behind a whole chunk that its e_r reaches: the partial of that
//                (row, chunk) is l = 0, Oc = 0, m = -1e30 + 8 -- finite, weight 0 in the combine.
//   direct form  NCw == 1: the sweep kernel merges its two streams through the stage LDS, adds the sink term and stores O
//                as v4f itself -- one launch, no scratch traffic (a 128-key window is five or six tiles; a second launch
//                would cost more than the sweep).  It also writes an invalid sequence's zeros.
//   combine      NCw > 1: qmha_fp8_decode_window_combine_kernel, qmha_split_combine_kernel's arithmetic in its order over
//                the chunks 0 ... (e_r / 32 - t0) / C, the sink term added to Ltot last.
//   sink         head k's softmax has one more column sinks[k] (natural-log units of S / sqrt(d)) with no value row:
//                O = sum p_j v_j / (sum p_j + 2^(sink log2(e) - m + 8)), the 2^8 the bias l carries.  The exponent is
//                clamped at 120 before exp2, so the term is finite whatever the sink; a sink that far above the row's
//                maximum leaves |O| below 2^-100 max|v| either way.
// A stream's arithmetic, the merge of the two streams and the partial a chunk writes are qmha_fp8_decode.hip's, statement for
// statement: with window >= L and no sinks the combine form's O is that call's, bit for bit.
// No atomics, no flags, no waiting on another workgroup: one or two plain launches on one stream.
#include "qmha_fa_masked.hpp"
#include "qmha_fp8.hpp"

#include <limits.h>

namespace qmha {

// where the results go and how the sweep is cut: C tiles per chunk (even), NC = NCw chunks
struct DecodeWindowOut {
    float *Oc, *pm, *pl;  // [B][NC][Nq][h D], [B][NC][Nq][h], [B][NC][Nq][h]; the direct form uses none
    float* O;             // [B][Nq][h D]
    const float* sinks;   // DEVICE float32 [h], or null
    int C, NC, window;
};

// 2^(sink log2(e) - m + 8) for a maximum given less its bias of 8, the exponent clamped: finite for every finite sink
__device__ __forceinline__ float sink_term(float sink, float m_less_bias) {
    return __builtin_amdgcn_exp2f(fminf(sink * kLog2e - m_less_bias, 120.0f));
}
// the first tile of a sequence's sweep: the two-tile stage that holds the first key row 0 sees
__device__ __forceinline__ int window_t0(int L, int Nq, int window) { return max(0, L - Nq - window + 1) / (kSG * QMHA_GROUP) * kSG; }

template <class Geo, int D, int QB, bool DIRECT>
__global__ __launch_bounds__(kWaves * 64, D > 64 ? 2 : 4) void qmha_fp8_decode_window_kernel(
    const float* __restrict__ Qf, const uint8_t* __restrict__ K8, const uint8_t* __restrict__ Vt8, Geo any, DecodeWindowOut out,
    const int32_t* __restrict__ lens, int H, int d_model, float q_scale, float s_log2, float v_scale) {
    static_assert(kRaggedGeo<Geo> && !kSplitGeo<Geo> && !kPackedGeo<Geo> && !kWindowGeo<Geo>, "Ragged or Paged");
    static_assert(kWaves == 4 && kSG == 2, "wave w is (tile w & 1 of the stage, d-half w >> 1)");
    // the workgroup's (K/V slice, chunk) and the sequence's verdict: workgroup-uniform, before the first barrier or DMA
    // issue.  An invalid sequence writes nothing here in the combine form (the combine kernel writes its zeros); the direct
    // form, whose only chunk is 0, zeroes the G heads' columns of its rows.  A chunk behind the last tile leaves.
    int bh, qb_, c;
    split_wg(1, out.NC, bh, qb_, c);
    const int b = bh / H, kvh = bh % H;  // bh: the K/V slice (H K/V heads)
    const int Nq = any.Nq, G = any.G;
    const int L = __builtin_amdgcn_readfirstlane(lens[b]);
    bool valid = any.valid(L);  // Nq <= L <= cap
    const int t0 = valid ? window_t0(L, Nq, out.window) : 0;
    if constexpr (kPagedGeo<Geo>) {
        if (valid) valid = any.used_pages_ok(b, t0 * QMHA_GROUP, L);
    }
    if (!valid) {
        if constexpr (DIRECT) zero_real_rows<D>(out.O, any, bh, H, d_model);
        return;
    }
    const int t_first = t0 + c * out.C, t_last = (L - 1) / QMHA_GROUP;
    if (t_first > t_last) return;
    const int t_end = min(t_first + out.C - 1, t_last);  // the chunk's last tile: t_end / 2 < cap / 64

    asm volatile("" : "+v"(s_log2));  // a VOP3 fma reading an SGPR issues at the slow rate
    constexpr int WAVES = kWaves, SG = kSG;
    constexpr int KP = D / 64;            // 16-byte chunks a lane reads of a K row: two QK k-steps each
    constexpr int DB = D / 16;            // PV d-blocks of 16 rows, read in pairs
    constexpr int MH = DB / 2;            // the d-blocks of a wave: dh MH .. +MH - 1
    constexpr int RB = D;                 // K row bytes
    constexpr int KBYTES = SG * 32 * RB;  // K per stage
    constexpr int VBYTES = SG * 32 * D;   // V^T per stage
    constexpr int KCH = KBYTES / 16, VCH = VBYTES / 16;
    static_assert(D == 64 || D == 128, "fp8 cache: d in {64, 128}");
    static_assert(QB == 1 || QB == 2, "W <= 32 columns");
    static_assert(KCH % 64 == 0 && VCH % 64 == 0 && (KCH / SG) % 64 == 0 && (VCH / SG) % 64 == 0, "whole KiB LDS-DMA pieces");
    __shared__ __attribute__((aligned(16))) char lds[2][KBYTES + VBYTES];
    // the hand-over of a tp = 1 wave at the chunk's end: MH QB v4f of o and QB (m, l) pairs per lane, lane-interleaved
    constexpr int HAND = 64 * (MH * QB * 16 + QB * 8);
    static_assert(2 * HAND <= (int)sizeof(lds), "the hand-over fits the stage buffers");

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int tp = wave & 1, dh = wave >> 1;
    const int grp = lane >> 4, r16 = lane & 15;
    const int W = G * Nq, nst = (t_end - t_first) / SG + 1;

    // this lane's columns: (head, row), the last key the column sees and the last key it does not see on its left
    bool real[QB];
    int head[QB], row[QB], lim[QB], lolim[QB];
#pragma unroll
    for (int qb = 0; qb < QB; ++qb) {
        const int col = 16 * qb + r16;
        real[qb] = col < W;
        const int g = real[qb] ? (int)((unsigned)col / (unsigned)Nq) : 0;
        row[qb] = real[qb] ? col - g * Nq : 0;
        head[qb] = kvh * G + g;
        lim[qb] = L - Nq + row[qb];
        lolim[qb] = lim[qb] - out.window;  // >= -INT_MAX
    }
    // Q into the QK B operand: column 16 qb + r16, bytes d = 64 kp + 16 grp + 8 h .. +7 for k-step 2 kp + h
    fp8x8 qop[QB][2 * KP];
#pragma unroll
    for (int qb = 0; qb < QB; ++qb)
#pragma unroll
        for (int ks = 0; ks < 2 * KP; ++ks) {
            float x[8] = {};
            if (real[qb]) {  // a pad column loads nothing
                const float* qp = Qf + ((size_t)b * Nq + row[qb]) * d_model + (size_t)head[qb] * D + 64 * (ks >> 1) + 16 * grp + 8 * (ks & 1);
                const v4f a = *reinterpret_cast<const v4f*>(qp), e4 = *reinterpret_cast<const v4f*>(qp + 4);
#pragma unroll
                for (int e = 0; e < 4; ++e) x[e] = fp8_prep(a[e], q_scale), x[4 + e] = fp8_prep(e4[e], q_scale);
            }
            qop[qb][ks] = fp8_pack8(x);
        }
    v4f o[MH][QB];
#pragma unroll
    for (int m = 0; m < MH; ++m)
#pragma unroll
        for (int qb = 0; qb < QB; ++qb) o[m][qb] = v4f{};
    // mb: the stream's running maximum less the bias of 8 (log2 units); no score is below -1e30.  l: over this lane's keys
    float mb[QB], l_run[QB];
#pragma unroll
    for (int qb = 0; qb < QB; ++qb) mb[qb] = -1e30f, l_run[qb] = 0.0f;

    const int Nk = any.nk();
    const char* kbase = reinterpret_cast<const char*>(K8 + (size_t)bh * Nk * D);
    const char* vbase = reinterpret_cast<const char*>(Vt8 + (size_t)bh * Nk * D);
    MaskedStager<WAVES, KCH, VCH, KBYTES, VBYTES, SG> stg;
#pragma unroll
    for (int jj = 0; jj < stg.KJ; ++jj) {
        const int idx = (wave + jj * WAVES) * 64 + lane;
        const int krow = idx / (RB / 16), cc = (idx % (RB / 16)) ^ kswz16<RB>(krow);
        stg.koff[jj] = krow * RB + 16 * cc;
    }
#pragma unroll
    for (int jj = 0; jj < stg.VJ; ++jj) {
        const int idx = (wave + jj * WAVES) * 64 + lane;
        const int gq = idx / (2 * D), w = idx % (2 * D);
        const int line = w >> 2, cv = (w & 3) ^ vswz16(line);
        stg.voff[jj] = gq * 32 * D + line * 64 + 16 * cv;
    }
    // stage st of the chunk is stage t_first / 2 + st of the sequence (t_first is even: t0 and C are).  Paged: the stage's
    // page slice is the buffer, the stage offset the stage's place in its page; the walk starts at the chunk's first tile,
    // whose column and every later one up to L's passed used_pages_ok.  Only tiles <= t_end come in.
    std::conditional_t<kPagedGeo<Geo>, PageWalk, NoWalk> walk;
    if constexpr (kPagedGeo<Geo>) walk.start_at(any, b, t_first);
    auto issue = [&](int buf, int st) {
        const int ts = t_first + st * SG, ngr = min(SG, t_end + 1 - ts);
        if constexpr (kPagedGeo<Geo>) {
            walk.take(any);
            const size_t slice = (size_t)walk.page * H + kvh, pbytes = (size_t)any.PG * (QMHA_GROUP * D);
            stg.issue(lds[buf], reinterpret_cast<const char*>(K8) + slice * pbytes, (int)pbytes,
                      reinterpret_cast<const char*>(Vt8) + slice * pbytes, (int)pbytes, walk.sip, ngr, wave);
            walk.advance(any, b);
        } else
            stg.issue(lds[buf], kbase, Nk * RB, vbase, Nk * D, ts / SG, ngr, wave);
    };
    // S^T blocks [kb][qb] of this wave's tile of the stage: rows kap16(kb, .) of the K tile against column block qb
    struct S2 {
        v4f v[2][QB];
    };
    auto qk = [&](const char* Lb) {
        S2 s;
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
            const int krow = tp * 32 + kap16(kb, r16);
#pragma unroll
            for (int qb = 0; qb < QB; ++qb) s.v[kb][qb] = v4f{};
#pragma unroll
            for (int kp = 0; kp < KP; ++kp) {
                const v2l kop = *reinterpret_cast<const v2l*>(Lb + krow * RB + 16 * ((4 * kp + grp) ^ kswz16<RB>(krow)));
#pragma unroll
                for (int h = 0; h < 2; ++h)
#pragma unroll
                    for (int qb = 0; qb < QB; ++qb)
                        s.v[kb][qb] = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(kop[h], qop[qb][2 * kp + h], s.v[kb][qb], 0, 0, 0);
            }
        }
        return s;
    };
    const int key0 = kap16(0, 4 * grp);  // this lane's keys of a tile: key0 + i + 8 kb
    auto tile = [&](const char* Lb, int t, S2 s) {
        v2l vop[MH / 2];  // V^T rows 32 mp + r16 and + 16 of this wave's d-half, slots 8 grp .. +7
#pragma unroll
        for (int mi = 0; mi < MH / 2; ++mi) {
            const int line = 16 * (dh * (MH / 2) + mi) + r16;
            vop[mi] = *reinterpret_cast<const v2l*>(Lb + KBYTES + tp * 32 * D + line * 64 + 16 * (grp ^ vswz16(line)));
        }
        if (32 * t + 31 > L - Nq) {  // wave-uniform: the tile holds a key some column does not see yet
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int qb = 0; qb < QB; ++qb)
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        s.v[kb][qb][i] = 32 * t + key0 + i + 8 * kb > lim[qb] ? -__builtin_huge_valf() : s.v[kb][qb][i];
        }
        if (32 * t <= L - 1 - out.window) {  // wave-uniform: the tile holds a key some column sees no more
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int qb = 0; qb < QB; ++qb)
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        s.v[kb][qb][i] = 32 * t + key0 + i + 8 * kb <= lolim[qb] ? -__builtin_huge_valf() : s.v[kb][qb][i];
        }
        float sc[QB][8], mx[QB];
        bool rises = false;
#pragma unroll
        for (int qb = 0; qb < QB; ++qb) {
#pragma unroll
            for (int j = 0; j < 8; ++j) sc[qb][j] = s.v[j >> 2][qb][j & 3] * s_log2;  // masked: -inf
            mx[qb] = fmaxf(fmaxf(fmaxf(sc[qb][0], sc[qb][1]), fmaxf(sc[qb][2], sc[qb][3])),
                           fmaxf(fmaxf(sc[qb][4], sc[qb][5]), fmaxf(sc[qb][6], sc[qb][7])));
            rises |= mx[qb] - 8.0f > mb[qb];
        }
        if (__builtin_amdgcn_ballot_w64(rises)) {  // wave-uniform: some column's maximum rises
#pragma unroll
            for (int qb = 0; qb < QB; ++qb) {
                float r = mx[qb];  // the column's four lane groups
                r = fmaxf(r, __shfl_xor(r, 16));
                r = fmaxf(r, __shfl_xor(r, 32));
                const float m_b = fmaxf(mb[qb], r - 8.0f);
                const float alpha = __builtin_amdgcn_exp2f(mb[qb] - m_b);  // 1 for a column that stays
                l_run[qb] *= alpha;
#pragma unroll
                for (int m = 0; m < MH; ++m) o[m][qb] *= alpha;
                mb[qb] = m_b;
            }
        }
#pragma unroll
        for (int qb = 0; qb < QB; ++qb) {
            float p[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) p[j] = __builtin_amdgcn_exp2f(sc[qb][j] - mb[qb]);  // <= 2^8; masked: 0
            l_run[qb] += ((p[0] + p[1]) + (p[2] + p[3])) + ((p[4] + p[5]) + (p[6] + p[7]));
            const fp8x8 pop = fp8_pack8(p);
#pragma unroll
            for (int m = 0; m < MH; ++m) o[m][qb] = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(vop[m >> 1][m & 1], pop, o[m][qb], 0, 0, 0);
        }
    };

    issue(0, 0);
    qmha_dma_barrier();
    auto stage = [&](auto BUF, int st) {
        constexpr int buf = decltype(BUF)::value;
        if (st + 1 < nst) issue(buf ^ 1, st + 1);
        const int t = t_first + st * SG + tp;
        if (t <= t_end) tile(lds[buf], t, qk(lds[buf]));  // wave-uniform
        qmha_dma_barrier();
    };
    int st = 0;
    for (; st + 2 <= nst; st += 2) {
        stage(std::integral_constant<int, 0>{}, st);
        stage(std::integral_constant<int, 1>{}, st + 1);
    }
    if (st < nst) stage(std::integral_constant<int, 0>{}, st);

    // The chunk's end.  Behind the last barrier no DMA is in flight and no wave reads a stage any more: the odd stream's
    // waves put their state into the stage buffers, the even stream's waves of the same d-half merge and store.
#pragma unroll
    for (int qb = 0; qb < QB; ++qb) {
        l_run[qb] += __shfl_xor(l_run[qb], 16);
        l_run[qb] += __shfl_xor(l_run[qb], 32);
    }
    char* hand = &lds[0][0] + dh * HAND;
    if (tp == 1) {
#pragma unroll
        for (int m = 0; m < MH; ++m)
#pragma unroll
            for (int qb = 0; qb < QB; ++qb) *reinterpret_cast<v4f*>(hand + ((m * QB + qb) * 64 + lane) * 16) = o[m][qb];
#pragma unroll
        for (int qb = 0; qb < QB; ++qb) *reinterpret_cast<v2f*>(hand + MH * QB * 64 * 16 + (qb * 64 + lane) * 8) = v2f{mb[qb], l_run[qb]};
    }
    __syncthreads();
    if (tp == 1) return;
    const int h = H * G;
#pragma unroll
    for (int qb = 0; qb < QB; ++qb) {
        const v2f ml = *reinterpret_cast<const v2f*>(hand + MH * QB * 64 * 16 + (qb * 64 + lane) * 8);
        const float M = fmaxf(mb[qb], ml[0]);
        const float w0 = __builtin_amdgcn_exp2f(mb[qb] - M), w1 = __builtin_amdgcn_exp2f(ml[0] - M);  // an empty stream: 0 (or l = 0)
        const float l = w0 * l_run[qb] + w1 * ml[1];
        if constexpr (DIRECT) {
            // the only chunk: every real row has its own key e_r in it.  The sink joins the row sum, then O itself
            if (!real[qb]) continue;
            const float lt = out.sinks ? l + sink_term(out.sinks[head[qb]], M) : l;
            const bool ok = lt > 1e-10f;
            float* orow = out.O + ((size_t)b * Nq + row[qb]) * d_model + (size_t)head[qb] * D + 16 * (dh * MH) + 4 * grp;
#pragma unroll
            for (int m = 0; m < MH; ++m) {
                const v4f o1 = *reinterpret_cast<const v4f*>(hand + ((m * QB + qb) * 64 + lane) * 16);
                v4f w;
#pragma unroll
                for (int j = 0; j < 4; ++j) w[j] = ok ? v_scale * ((w0 * o[m][qb][j] + w1 * o1[j]) / lt) : 0.0f;
                *reinterpret_cast<v4f*>(orow + 16 * m) = w;
            }
        } else {
            const bool ok = l > 1e-10f;  // false: no key of the chunk is visible to the row -- l = 0, Oc = 0, m = -1e30 + 8
            // row r writes chunk c iff c <= ((L - Nq + r) / 32 - t0) / C: what the combine reads of it
            if (!real[qb] || c > (lim[qb] / QMHA_GROUP - t0) / out.C) continue;
            const size_t at = ((size_t)b * out.NC + c) * Nq + row[qb];
            float* orow = out.Oc + at * d_model + (size_t)head[qb] * D + 16 * (dh * MH) + 4 * grp;
#pragma unroll
            for (int m = 0; m < MH; ++m) {
                const v4f o1 = *reinterpret_cast<const v4f*>(hand + ((m * QB + qb) * 64 + lane) * 16);
                v4f w;
#pragma unroll
                for (int j = 0; j < 4; ++j) w[j] = ok ? v_scale * ((w0 * o[m][qb][j] + w1 * o1[j]) / l) : 0.0f;
                *reinterpret_cast<v4f*>(orow + 16 * m) = w;
            }
            if (dh == 0 && grp == 0) {
                out.pl[at * h + head[qb]] = l;
                out.pm[at * h + head[qb]] = M + 8.0f;  // the true maximum
            }
        }
    }
}

// The combine pass: a thread per 16 bytes of a real row of O, qmha_split_combine_kernel's arithmetic in its order.  Row r of
// sequence b, head k reads the chunks c = 0 ... ((L - Nq + r) / 32 - t0) / C -- the ones the sweep wrote for it, and nothing
// else of the scratch --, ascending, in fp32:  M = max m_c,  a_c = l_c 2^(m_c - M),  Ltot = sum a_c, then the sink's
// 2^(sink log2(e) - M + 8);  O = Ltot > thr ? (sum a_c Oc_c) / Ltot : 0.  An invalid sequence (a length outside [Nq, cap]; a
// table entry outside the pool among the columns of rows [32 t0, L)): positive zeros, no scratch read.  table null: a
// contiguous cache, no entry is looked at.
__global__ __launch_bounds__(256) void qmha_fp8_decode_window_combine_kernel(Paged any, DecodeWindowOut out, const int32_t* __restrict__ lens,
                                                                             int h, int D, float thr) {
    const int W4 = h * D / 4;  // 16-byte pieces of a row
    const unsigned per = ((unsigned)any.Nq * (unsigned)W4 + 255u) / 256u;  // blocks of a sequence
    const int b = (int)(blockIdx.x / per);
    const int L = lens[b];
    bool valid = any.valid(L);
    const int t0 = valid ? window_t0(L, any.Nq, out.window) : 0;
    if (valid && any.table) valid = any.used_pages_ok(b, t0 * QMHA_GROUP, L);  // block-uniform: every lane takes part in the ballot
    const int i = (int)(blockIdx.x % per) * 256 + threadIdx.x;
    if (i >= any.Nq * W4) return;
    const int r = i / W4, w = i % W4, k = w / (D / 4);
    float* o = out.O + ((size_t)b * any.Nq + r) * ((size_t)h * D) + 4 * w;
    if (!valid) {
        *reinterpret_cast<v4f*>(o) = v4f{};
        return;
    }
    const int n = ((L - any.Nq + r) / QMHA_GROUP - t0) / out.C + 1;  // <= NC: the sweep is at most NC C tiles
    const size_t step = (size_t)any.Nq * h, at = ((size_t)b * out.NC * any.Nq + r) * h + k;  // chunk c: at + c step
    float M = out.pm[at];
    for (int c = 1; c < n; ++c) M = fmaxf(M, out.pm[at + c * step]);
    float Ltot = 0.0f;
    v4f acc = v4f{};
    for (int c = 0; c < n; ++c) {
        const float a = out.pl[at + c * step] * __builtin_amdgcn_exp2f(out.pm[at + c * step] - M);
        const v4f oc = *reinterpret_cast<const v4f*>(out.Oc + (((size_t)b * out.NC + c) * any.Nq + r) * ((size_t)h * D) + 4 * w);
        Ltot += a;
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] = fmaf(a, oc[e], acc[e]);
    }
    if (out.sinks) Ltot += sink_term(out.sinks[k], M - 8.0f);
    v4f res;
#pragma unroll
    for (int e = 0; e < 4; ++e) res[e] = Ltot > thr ? acc[e] / Ltot : 0.0f;
    *reinterpret_cast<v4f*>(o) = res;
}

// ---------------------------------------------------------------------------------------
// host: masked_geo's Ragged / Paged geometry of a token-granular call; QB from W = Nq * (H / Hkv); the form from the chunks
// ---------------------------------------------------------------------------------------
template <class Geo>
static hipError_t fp8_decode_window_launch(const Fp8Workspace& w, const float* Qf, float* O, const MaskedCall& c, int window, const float* sinks,
                                           int chunk_rows, void* scratch, hipStream_t stream, Geo geo) {
    const int W = c.Nq * (c.H / c.Hkv);
    if (!scratch || window < 1 || W > 32 || chunk_rows < 2 * QMHA_GROUP || chunk_rows % (2 * QMHA_GROUP) != 0 || chunk_rows > c.Nk)
        return hipErrorInvalidValue;
    const int NC = decode_window_chunks(c.Nk, c.Nq, window, chunk_rows);
    if ((long long)c.B * c.Hkv * NC > INT_MAX || ((long long)c.Nq * c.d_model / 4 + 255) / 256 * c.B > INT_MAX) return hipErrorInvalidValue;
    const SplitScratch s = split_carve(scratch, c.B, NC, c.Nq, c.H, c.D);
    const DecodeWindowOut out{s.Oc, s.m, s.l, O, sinks, chunk_rows / QMHA_GROUP, NC, window};
    const dim3 grid(c.B * c.Hkv * NC), block(kWaves * 64);
    const hipError_t e = fp8_cache_d(c.D, [&](auto d) {
        auto go = [&](auto qb, auto direct) {
            hipLaunchKernelGGL((qmha_fp8_decode_window_kernel<Geo, decltype(d)::value, decltype(qb)::value, decltype(direct)::value>), grid, block, 0,
                               stream, Qf, w.K8, w.Vt8, geo, out, c.lens, c.Hkv, c.d_model, w.q_scale,
                               w.q_scale * w.k_scale * softmax_scale_log2(c.D), w.v_scale);
            return hipGetLastError();
        };
        auto form = [&](auto qb) { return NC == 1 ? go(qb, std::true_type{}) : go(qb, std::false_type{}); };
        return W > 16 ? form(std::integral_constant<int, 2>{}) : form(std::integral_constant<int, 1>{});
    });
    if (e != hipSuccess || NC == 1) return e;
    const dim3 cgrid((unsigned)(((size_t)c.Nq * c.d_model / 4 + 255) / 256 * c.B));
    hipLaunchKernelGGL(qmha_fp8_decode_window_combine_kernel, cgrid, dim3(256), 0, stream, as_paged(geo), out, c.lens, c.H, c.D, 1e-10f);
    return hipGetLastError();
}

hipError_t launch_fp8_decode_window(const Fp8Workspace& w, const float* Qf, float* O, const MaskedCall& c, int window, const float* sinks,
                                    int chunk_rows, void* scratch, hipStream_t stream) {
    if (!c.ragged) return hipErrorInvalidValue;
    return masked_geo(c, [&](auto geo) {
        if constexpr (kRaggedGeo<decltype(geo)>) return fp8_decode_window_launch(w, Qf, O, c, window, sinks, chunk_rows, scratch, stream, geo);
        else return hipErrorInvalidValue;
    });
}

}  // namespace qmha
