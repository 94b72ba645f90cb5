// qmha_fp8_shared.hip -- the shared-prefix decode call of an e4m3 K/V cache (fa_tc_fp8) for gfx950 (MI355X), in
// a translation unit of its own so that every other kernel keeps its bytes.  qmha_fp8_decode.hip sweeps each sequence's keys
// on their own and fills at most 32 MFMA columns with one sequence's G Nq query rows.  Where the first P = prefix_rows cache
// rows of every sequence are those of slot 0 -- a system prompt stored once --, this call sweeps them once for the batch:
//   prefix item   (K/V head, prefix chunk c < P / chunk_rows, column group).  The columns are all B W query rows of the batch
//                 that belong to the K/V head, W = G Nq: column cidx = b W + g Nq + r is sequence b, query head kvh G + g, row
//                 r.  A workgroup takes QB 16-column blocks of them; a block may straddle two sequences.  Every prefix key is
//                 seen by every column (P <= lens[b] - Nq), so the path has no mask and no select.  Each K and V^T operand a
//                 wave reads from LDS feeds QB MFMAs.  Column cidx's (O, m, l) goes to slot [b][c][r][head] of the scratch.
//   suffix item   (sequence, K/V head, chunk c >= P / chunk_rows): the decode kernel's body with its mask over the sequence's
//                 own rows.  A chunk that starts behind the sequence's last tile returns.
//   one launch    over the flattened items, the prefix items first (they are whole chunks, the long ones), then the combine.
// MFMA columns do not interact and a prefix chunk is a whole chunk of decode's chunk grid, so chunk c of sequence b has the
// partial decode writes for it on a cache that holds a copy of the prefix in every slice, in the same SplitScratch slot; the
// combine kernel here is qmha_split_combine_kernel's arithmetic in its order.  It is this unit's own for the verdict alone:
// that kernel tests every used table column of sequence b, where this call promises not to look at the columns that hold
// only prefix rows (they may be -1), and it would join stale partials for a sequence whose lens[b] is a decode length but
// whose rows do not reach the prefix's end, where this call gives zeros.
//   verdict       sequence b takes part iff Nq <= lens[b] <= cap, P <= lens[b] - Nq, (paged) the entries of table row 0 that
//                 hold prefix rows lie in the pool, and so do those of row b that hold a row in [P, lens[b]).  The combine
//                 kernel applies all of it and writes positive zeros otherwise.  A prefix item stops on a bad prefix entry
//                 and drops the columns whose length fails; a suffix item applies the sequence's own part.  A workgroup
//                 that computes a partial the combine does not read only fills scratch of its own slot.
// The stages, the wave roles (tp, dh), the stream arithmetic, the stream merge and the stores are qmha_fp8_decode.hip's, kept
// word for word: Q through fp8_prep / q_scale, S on v_mfma_f32_16x16x32_fp8_fp8, the ballot-guarded running maximum, p =
// exp2(s - m + 8) through v_cvt_pk_fp8_f32, the fp32 merge of the even and the odd stream.
// No atomics, no flags, no waiting on another workgroup: two plain launches on one stream.
#include "qmha_fa_masked.hpp"
#include "qmha_fp8.hpp"

#include <limits.h>

namespace qmha {

// where the partials go (split_carve's arrays) and how the work is cut: C tiles per chunk (even), NC chunks of the cache, of
// which the first PC are the prefix's; NG column groups of a prefix chunk over the batch's B sequences; P = prefix_rows
struct SharedOut {
    float *Oc, *pm, *pl;  // [B][NC][Nq][h D], [B][NC][Nq][h], [B][NC][Nq][h]
    int C, NC, PC, NG, B, P;
};

// a lane's columns: sequence, query head, row, and the last key the column sees
template <int QB>
struct SharedCols {
    bool real[QB];
    int b[QB], head[QB], row[QB], lim[QB];
};

constexpr int shared_stage_bytes(int D) { return kSG * 32 * D * 2; }  // K and V^T of a two-tile stage

// The sweep of tiles t_first .. t_end of K/V head kvh, rows of sequence slot sb (a prefix item: 0), for the columns `col`, and
// the store of each real column's partial of chunk c.  kMask: the decode call's mask, Lm = L - Nq of the one sequence the
// columns belong to; else every column sees every key of the sweep.
template <class Geo, int D, int QB, bool kMask>
__device__ __forceinline__ void shared_sweep(char* lds, const float* __restrict__ Qf, const uint8_t* __restrict__ K8,
                                             const uint8_t* __restrict__ Vt8, const Geo& any, const SharedOut& out, const SharedCols<QB>& col,
                                             int sb, int kvh, int c, int t_first, int t_end, int Lm, int H, int d_model, float q_scale,
                                             float s_log2, float v_scale) {
    constexpr int WAVES = kWaves, SG = kSG;
    constexpr int KP = D / 64;            // 16-byte chunks a lane reads of a K row: two QK k-steps each
    constexpr int DB = D / 16;            // PV d-blocks of 16 rows, read in pairs
    constexpr int MH = DB / 2;            // the d-blocks of a wave: dh MH .. +MH - 1
    constexpr int RB = D;                 // K row bytes
    constexpr int KBYTES = SG * 32 * RB;  // K per stage
    constexpr int VBYTES = SG * 32 * D;   // V^T per stage
    constexpr int KCH = KBYTES / 16, VCH = VBYTES / 16;
    constexpr int STAGE = KBYTES + VBYTES;
    static_assert(STAGE == shared_stage_bytes(D), "the kernel's LDS block");
    static_assert(KCH % 64 == 0 && VCH % 64 == 0 && (KCH / SG) % 64 == 0 && (VCH / SG) % 64 == 0, "whole KiB LDS-DMA pieces");
    // the hand-over of a tp = 1 wave at the chunk's end: MH QB v4f of o and QB (m, l) pairs per lane, lane-interleaved
    constexpr int HAND = 64 * (MH * QB * 16 + QB * 8);
    static_assert(2 * HAND <= 2 * STAGE, "the hand-over fits the stage buffers");

    asm volatile("" : "+v"(s_log2));  // a VOP3 fma reading an SGPR issues at the slow rate
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int tp = wave & 1, dh = wave >> 1;
    const int grp = lane >> 4, r16 = lane & 15;
    const int Nq = any.Nq, nst = (t_end - t_first) / SG + 1;

    // Q into the QK B operand: the lane's column of block qb, bytes d = 64 kp + 16 grp + 8 h .. +7 for k-step 2 kp + h
    fp8x8 qop[QB][2 * KP];
#pragma unroll
    for (int qb = 0; qb < QB; ++qb)
#pragma unroll
        for (int ks = 0; ks < 2 * KP; ++ks) {
            float x[8] = {};
            if (col.real[qb]) {  // a pad column or a left-out sequence's loads nothing
                const float* qp = Qf + ((size_t)col.b[qb] * Nq + col.row[qb]) * d_model + (size_t)col.head[qb] * D + 64 * (ks >> 1) + 16 * grp + 8 * (ks & 1);
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
    const size_t bh = (size_t)sb * H + kvh;
    const char* kbase = reinterpret_cast<const char*>(K8 + bh * Nk * D);
    const char* vbase = reinterpret_cast<const char*>(Vt8 + bh * Nk * D);
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
    // stage st of the sweep is stage t_first / 2 + st of slot sb.  Paged: the stage's page slice is the buffer, the stage
    // offset the stage's place in its page; the walk starts at the sweep's first tile, in table row sb.  Only tiles <= t_end
    // come in.
    std::conditional_t<kPagedGeo<Geo>, PageWalk, NoWalk> walk;
    if constexpr (kPagedGeo<Geo>) walk.start_at(any, sb, t_first);
    auto issue = [&](int buf, int st) {
        const int t0 = t_first + st * SG, ngr = min(SG, t_end + 1 - t0);
        if constexpr (kPagedGeo<Geo>) {
            walk.take(any);
            const size_t slice = (size_t)walk.page * H + kvh, pbytes = (size_t)any.PG * (QMHA_GROUP * D);
            stg.issue(lds + buf * STAGE, reinterpret_cast<const char*>(K8) + slice * pbytes, (int)pbytes,
                      reinterpret_cast<const char*>(Vt8) + slice * pbytes, (int)pbytes, walk.sip, ngr, wave);
            walk.advance(any, sb);
        } else
            stg.issue(lds + buf * STAGE, kbase, Nk * RB, vbase, Nk * D, t0 / SG, ngr, wave);
    };
    // S^T blocks [kb][qb] of this wave's tile of the stage: rows kap16(kb, .) of the K tile against column block qb.  One
    // ds_read_b128 of K feeds 2 QB MFMAs.
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
        v2l vop[MH / 2];  // V^T rows 32 mp + r16 and + 16 of this wave's d-half, slots 8 grp .. +7: each feeds 2 QB MFMAs
#pragma unroll
        for (int mi = 0; mi < MH / 2; ++mi) {
            const int line = 16 * (dh * (MH / 2) + mi) + r16;
            vop[mi] = *reinterpret_cast<const v2l*>(Lb + KBYTES + tp * 32 * D + line * 64 + 16 * (grp ^ vswz16(line)));
        }
        if constexpr (kMask) {
            if (32 * t + 31 > Lm) {  // wave-uniform: the tile holds a key some column does not see
#pragma unroll
                for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                    for (int qb = 0; qb < QB; ++qb)
#pragma unroll
                        for (int i = 0; i < 4; ++i)
                            s.v[kb][qb][i] = 32 * t + key0 + i + 8 * kb > col.lim[qb] ? -__builtin_huge_valf() : s.v[kb][qb][i];
            }
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
        if (t <= t_end) tile(lds + buf * STAGE, t, qk(lds + buf * STAGE));  // wave-uniform
        qmha_dma_barrier();
    };
    int st = 0;
    for (; st + 2 <= nst; st += 2) {
        stage(std::integral_constant<int, 0>{}, st);
        stage(std::integral_constant<int, 1>{}, st + 1);
    }
    if (st < nst) stage(std::integral_constant<int, 0>{}, st);

    // The sweep's end.  Behind the last barrier no DMA is in flight and no wave reads a stage any more: the odd stream's
    // waves put their state into the stage buffers, the even stream's waves of the same d-half merge and store.
#pragma unroll
    for (int qb = 0; qb < QB; ++qb) {
        l_run[qb] += __shfl_xor(l_run[qb], 16);
        l_run[qb] += __shfl_xor(l_run[qb], 32);
    }
    char* hand = lds + dh * HAND;
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
    const int h = H * any.G;
#pragma unroll
    for (int qb = 0; qb < QB; ++qb) {
        const v2f ml = *reinterpret_cast<const v2f*>(hand + MH * QB * 64 * 16 + (qb * 64 + lane) * 8);
        const float M = fmaxf(mb[qb], ml[0]);
        const float w0 = __builtin_amdgcn_exp2f(mb[qb] - M), w1 = __builtin_amdgcn_exp2f(ml[0] - M);  // an empty stream: 0 (or l = 0)
        // the decode kernel's contractions, spelled out: which product of a sum of two is fused decides the last bit
        const float l = fmaf(w0, l_run[qb], w1 * ml[1]);
        const bool ok = l > 1e-10f;
        // row r writes chunk c iff c <= ((L - Nq + r) / 32) / C: what the combine reads of it.  A prefix chunk: always
        if (!col.real[qb]) continue;
        if constexpr (kMask) {
            if (c > col.lim[qb] / QMHA_GROUP / out.C) continue;
        }
        const size_t at = ((size_t)col.b[qb] * out.NC + c) * Nq + col.row[qb];
        float* orow = out.Oc + at * d_model + (size_t)col.head[qb] * D + 16 * (dh * MH) + 4 * grp;
#pragma unroll
        for (int m = 0; m < MH; ++m) {
            const v4f o1 = *reinterpret_cast<const v4f*>(hand + ((m * QB + qb) * 64 + lane) * 16);
            v4f w;
#pragma unroll
            for (int j = 0; j < 4; ++j) w[j] = ok ? v_scale * (fmaf(w1, o1[j], w0 * o[m][qb][j]) / l) : 0.0f;
            *reinterpret_cast<v4f*>(orow + 16 * m) = w;
        }
        if (dh == 0 && grp == 0) {
            out.pl[at * h + col.head[qb]] = l;
            out.pm[at * h + col.head[qb]] = M + 8.0f;  // the true maximum
        }
    }
}

// QBP: the 16-column blocks of a prefix item's column group.  QBS = ceil(W / 16): those of a suffix item.
template <class Geo, int D, int QBP, int QBS>
__global__ __launch_bounds__(kWaves * 64, D > 64 ? 2 : 4) void qmha_fp8_shared_kernel(
    const float* __restrict__ Qf, const uint8_t* __restrict__ K8, const uint8_t* __restrict__ Vt8, Geo any, SharedOut out,
    const int32_t* __restrict__ lens, int H, int d_model, float q_scale, float s_log2, float v_scale) {
    static_assert(kRaggedGeo<Geo> && !kSplitGeo<Geo> && !kPackedGeo<Geo> && !kWindowGeo<Geo>, "Ragged or Paged");
    static_assert(kWaves == 4 && kSG == 2, "wave w is (tile w & 1 of the stage, d-half w >> 1)");
    static_assert(D == 64 || D == 128, "fp8 cache: d in {64, 128}");
    static_assert((QBP == 1 || QBP == 2) && (QBS == 1 || QBS == 2) && QBS <= QBP, "W <= 32 columns; a group of one or two blocks");
    __shared__ __attribute__((aligned(16))) char lds[2 * shared_stage_bytes(D)];
    const int r16 = threadIdx.x & 15;
    const int Nq = any.Nq, G = any.G, W = G * Nq;
    const unsigned n_prefix = (unsigned)(H * out.PC * out.NG);
    // the item and its verdict: workgroup-uniform, before the first barrier or DMA issue
    if (blockIdx.x < n_prefix) {
        // a prefix item.  The groups of a chunk are neighbours: they read the same K/V
        const unsigned p = blockIdx.x, per = (unsigned)(out.PC * out.NG);
        const int kvh = (int)(p / per), c = (int)(p % per / (unsigned)out.NG), cg = (int)(p % (unsigned)out.NG);
        if constexpr (kPagedGeo<Geo>) {
            if (!any.used_pages_ok(0, out.P)) return;  // a prefix entry outside the pool: every sequence is left out
        }
        SharedCols<QBP> col;
        bool some = false;
#pragma unroll
        for (int qb = 0; qb < QBP; ++qb) {
            const int cidx = 16 * (QBP * cg + qb) + r16;
            const bool in = cidx < out.B * W;
            const int b = in ? (int)((unsigned)cidx / (unsigned)W) : 0;
            const int L = in ? lens[b] : 0;
            // the sequence's own words: a decode length that reaches the prefix's end
            col.real[qb] = in && L >= Nq && L <= any.Nk && L - Nq >= out.P;
            const int rem = col.real[qb] ? cidx - b * W : 0;
            const int g = (int)((unsigned)rem / (unsigned)Nq);
            col.b[qb] = col.real[qb] ? b : 0;
            col.row[qb] = rem - g * Nq;
            col.head[qb] = kvh * G + g;
            col.lim[qb] = L - Nq + col.row[qb];
            some |= col.real[qb];
        }
        if (!__builtin_amdgcn_ballot_w64(some)) return;  // the same columns in every wave: the same verdict
        const int t_first = c * out.C;                   // a whole chunk below P <= cap
        shared_sweep<Geo, D, QBP, false>(lds, Qf, K8, Vt8, any, out, col, 0, kvh, c, t_first, t_first + out.C - 1, 0, H, d_model, q_scale, s_log2,
                                         v_scale);
        return;
    }
    // a suffix item: the chunks of a K/V slice are neighbours, and xcd_remap keeps a slice's workgroups on one XCD
    const unsigned NS = (unsigned)(out.NC - out.PC);
    const unsigned wg = (unsigned)xcd_remap((int)(blockIdx.x - n_prefix), (int)(gridDim.x - n_prefix));
    const int bh = (int)(wg / NS), c = out.PC + (int)(wg % NS);
    const int b = bh / H, kvh = bh % H;
    const int L0 = lens[b];
    if (!any.valid(L0) || L0 - Nq < out.P) return;
    if constexpr (kPagedGeo<Geo>) {
        if (!any.used_pages_ok(b, out.P, L0)) return;  // the columns that hold a row in [P, L): the others are not looked at
    }
    const int L = __builtin_amdgcn_readfirstlane(L0);  // Nq + P <= L <= cap
    const int t_first = c * out.C, t_last = (L - 1) / QMHA_GROUP;
    if (t_first > t_last) return;
    const int t_end = min(t_first + out.C - 1, t_last);  // the chunk's last tile: t_end / 2 < cap / 64
    SharedCols<QBS> col;
#pragma unroll
    for (int qb = 0; qb < QBS; ++qb) {
        const int cc = 16 * qb + r16;
        col.real[qb] = cc < W;
        const int g = col.real[qb] ? (int)((unsigned)cc / (unsigned)Nq) : 0;
        col.b[qb] = b;
        col.row[qb] = col.real[qb] ? cc - g * Nq : 0;
        col.head[qb] = kvh * G + g;
        col.lim[qb] = L - Nq + col.row[qb];
    }
    shared_sweep<Geo, D, QBS, true>(lds, Qf, K8, Vt8, any, out, col, b, kvh, c, t_first, t_end, L - Nq, H, d_model, q_scale, s_log2, v_scale);
}

// The combine pass: a thread per 16 bytes of a real row of O, qmha_split_combine_kernel's arithmetic in its order over the
// chunks c = 0 ... last(qg) / C of the row's query group, under this call's verdict (the top of the file).  A sequence that
// is left out: positive zeros, no scratch read.  `any` is Split<Paged> for both kinds of cache; table null: a contiguous one.
__global__ __launch_bounds__(256) void qmha_fp8_shared_combine_kernel(float* __restrict__ O, Split<Paged> any, const int32_t* __restrict__ lens,
                                                                      int h, int D, float thr, int P) {
    const int W4 = h * D / 4;  // 16-byte pieces of a row
    const unsigned per = ((unsigned)any.Nq * (unsigned)W4 + 255u) / 256u;  // blocks of a sequence
    const int b = (int)(blockIdx.x / per);
    const int L = lens[b];
    bool valid = any.valid(L) && L - any.Nq >= P;
    // block-uniform: every lane takes part in the ballots
    if (valid && any.table) valid = any.used_pages_ok(0, P) && any.used_pages_ok(b, P, L);
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

// ---------------------------------------------------------------------------------------
// host: masked_geo's Ragged / Paged geometry of a token-granular call; QBS from W = Nq * (H / Hkv), QBP from the batch's
// column blocks; then the combine pass
// ---------------------------------------------------------------------------------------
template <class Geo>
static hipError_t fp8_shared_launch(const Fp8Workspace& w, const float* Qf, float* O, const MaskedCall& c, int prefix_rows, int chunk_rows,
                                    void* scratch, hipStream_t stream, Geo geo) {
    const int W = c.Nq * (c.H / c.Hkv);
    if (!scratch || W > 32 || chunk_rows < 2 * QMHA_GROUP || chunk_rows % (2 * QMHA_GROUP) != 0 || chunk_rows > c.Nk) return hipErrorInvalidValue;
    if (prefix_rows < chunk_rows || prefix_rows > c.Nk || prefix_rows % chunk_rows != 0) return hipErrorInvalidValue;
    const int NC = (c.Nk + chunk_rows - 1) / chunk_rows, PC = prefix_rows / chunk_rows;
    const long long blocks = ((long long)c.B * W + 15) / 16;  // 16-column blocks of a K/V head's columns
    const int qbp = blocks > 1 ? 2 : 1;
    const long long NG = (blocks + qbp - 1) / qbp, items = (long long)c.Hkv * PC * NG + (long long)c.B * c.Hkv * (NC - PC);
    if ((long long)c.B * W > INT_MAX || items > INT_MAX || ((long long)c.Nq * c.d_model / 4 + 255) / 256 * c.B > INT_MAX) return hipErrorInvalidValue;
    const SplitScratch s = split_carve(scratch, c.B, NC, c.Nq, c.H, c.D);
    const SharedOut out{s.Oc, s.m, s.l, chunk_rows / QMHA_GROUP, NC, PC, (int)NG, c.B, prefix_rows};
    const dim3 grid((unsigned)items), block(kWaves * 64);
    const hipError_t e = fp8_cache_d(c.D, [&](auto d) {
        auto go = [&](auto p, auto q) {
            hipLaunchKernelGGL((qmha_fp8_shared_kernel<Geo, decltype(d)::value, decltype(p)::value, decltype(q)::value>), grid, block, 0, stream, Qf,
                               w.K8, w.Vt8, geo, out, c.lens, c.Hkv, c.d_model, w.q_scale, w.q_scale * w.k_scale * softmax_scale_log2(c.D),
                               w.v_scale);
            return hipGetLastError();
        };
        using One = std::integral_constant<int, 1>;
        using Two = std::integral_constant<int, 2>;
        return W > 16 ? go(Two{}, Two{}) : qbp == 2 ? go(Two{}, One{}) : go(One{}, One{});  // W > 16: more than one block
    });
    if (e != hipSuccess) return e;
    const dim3 cgrid((unsigned)(((size_t)c.Nq * c.d_model / 4 + 255) / 256 * c.B)), cblock(256);
    hipLaunchKernelGGL(qmha_fp8_shared_combine_kernel, cgrid, cblock, 0, stream, O, Split<Paged>(as_paged(geo), s, out.C, NC), c.lens, c.H, c.D,
                       1e-10f, prefix_rows);
    return hipGetLastError();
}

hipError_t launch_fp8_decode_shared(const Fp8Workspace& w, const float* Qf, float* O, const MaskedCall& c, int prefix_rows, int chunk_rows,
                                    void* scratch, hipStream_t stream) {
    if (!c.ragged) return hipErrorInvalidValue;
    return masked_geo(c, [&](auto geo) {
        if constexpr (kRaggedGeo<decltype(geo)>) return fp8_shared_launch(w, Qf, O, c, prefix_rows, chunk_rows, scratch, stream, geo);
        else return hipErrorInvalidValue;
    });
}

}  // namespace qmha
