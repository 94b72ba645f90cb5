// qmha_fp8_decode.hip -- the decode call of an e4m3 K/V cache (fa_tc_fp8) for gfx950 (MI355X), in a
// translation unit of its own so that every other kernel keeps its bytes.  qmha_fa_fp8.hip's attend gives a wave a 32-row
// query group and lets it walk every key tile of the sequence; at a decode step one column of that block is real, the G
// query heads of a K/V head are G such waves, and the sweep is one long dependent chain.  This kernel turns the three
// around:
//   columns  the step's real query rows of one K/V head -- G heads x Nq rows, W = G Nq <= 32 -- are the columns of QB =
//            ceil(W / 16) MFMA blocks: column c = g Nq + r is query head kvh G + g, row r.  Columns >= W hold zeros, load
//            nothing and store nothing.
//   chunks   a workgroup is one (sequence, K/V head, chunk of C key tiles); it writes the chunk's partial (O, l, m) into
//            the caller's scratch, split-KV's layout (SplitScratch), and qmha_split_combine_kernel joins the chunks.
//   waves    the stages are qmha_fa_fp8.hip's: two key tiles by LDS-DMA, double-buffered, all four waves issuing.  Wave w
//            = (tp = w & 1, dh = w >> 1) takes tile tp of every stage -- the chunk's even tiles are one softmax stream,
//            its odd tiles another --, computes S^T = K Q^T and the stream's softmax for all QB blocks (the two dh waves
//            of a parity produce the same bits) and accumulates O^T = V^T P^T for the d-blocks of half dh only.  At the
//            chunk's end the tp = 1 waves hand (o, m, l) over through the stage LDS and the tp = 0 waves merge the two
//            streams in fp32 and store.
// The arithmetic of a stream is qmha_fa_fp8.hip's: Q through fp8_prep / q_scale, S on v_mfma_f32_16x16x32_fp8_fp8, the mask
// a select to -inf before the maximum (column (g, r) sees key j iff j <= L - Nq + r), the ballot-guarded TRUE running
// maximum, p = exp2(s - m + 8) through v_cvt_pk_fp8_f32 into P@V, l from the fp32 p.  The merge of streams 0 and 1:
// M = max(m0, m1), w_i = 2^(m_i - M), l = w0 l0 + w1 l1, Oc = l > 1e-10 ? v_scale (w0 o0 + w1 o1) / l : 0, m = M.
// No atomics, no flags, no waiting on another workgroup: two plain launches on one stream.
#include "qmha_fa_masked.hpp"
#include "qmha_fp8.hpp"

#include <limits.h>

namespace qmha {

// where the partials go (split_carve's arrays) and how the sweep is cut: C tiles per chunk (even), NC chunks
struct DecodeOut {
    float *Oc, *pm, *pl;  // [B][NC][Nq][h D], [B][NC][Nq][h], [B][NC][Nq][h]
    int C, NC;
};

template <class Geo, int D, int QB>
__global__ __launch_bounds__(kWaves * 64, D > 64 ? 2 : 4) void qmha_fp8_decode_kernel(
    const float* __restrict__ Qf, const uint8_t* __restrict__ K8, const uint8_t* __restrict__ Vt8, Geo any, DecodeOut out,
    const int32_t* __restrict__ lens, int H, int d_model, float q_scale, float s_log2, float v_scale) {
    static_assert(kRaggedGeo<Geo> && !kSplitGeo<Geo> && !kPackedGeo<Geo> && !kWindowGeo<Geo>, "Ragged or Paged");
    static_assert(kWaves == 4 && kSG == 2, "wave w is (tile w & 1 of the stage, d-half w >> 1)");
    // the workgroup's (K/V slice, chunk) and the sequence's verdict: workgroup-uniform, before the first barrier or DMA
    // issue.  An invalid sequence writes nothing here (the combine kernel writes its zeros), and neither does a chunk
    // that starts behind the sequence's last tile.
    int bh, qb_, c;
    split_wg(1, out.NC, bh, qb_, c);
    const int b = bh / H, kvh = bh % H;  // bh: the K/V slice (H K/V heads)
    const PackedSeq seq = cache_seq(any, lens, b);
    if (seq.verdict != 2) return;
    const int L = __builtin_amdgcn_readfirstlane(seq.L), Nq = any.Nq, G = any.G;  // Nq <= L <= cap
    const int t_first = c * out.C, t_last = (L - 1) / QMHA_GROUP;
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

    // this lane's columns: (head, row) and the last key the column sees
    bool real[QB];
    int head[QB], row[QB], lim[QB];
#pragma unroll
    for (int qb = 0; qb < QB; ++qb) {
        const int col = 16 * qb + r16;
        real[qb] = col < W;
        const int g = real[qb] ? (int)((unsigned)col / (unsigned)Nq) : 0;
        row[qb] = real[qb] ? col - g * Nq : 0;
        head[qb] = kvh * G + g;
        lim[qb] = L - Nq + row[qb];
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
    // stage st of the chunk is stage t_first / 2 + st of the sequence.  Paged: the stage's page slice is the buffer, the
    // stage offset the stage's place in its page; the walk starts at the chunk's first tile.  Only tiles <= t_end come in.
    std::conditional_t<kPagedGeo<Geo>, PageWalk, NoWalk> walk;
    if constexpr (kPagedGeo<Geo>) walk.start_at(any, b, t_first);
    auto issue = [&](int buf, int st) {
        const int t0 = t_first + st * SG, ngr = min(SG, t_end + 1 - t0);
        if constexpr (kPagedGeo<Geo>) {
            walk.take(any);
            const size_t slice = (size_t)walk.page * H + kvh, pbytes = (size_t)any.PG * (QMHA_GROUP * D);
            stg.issue(lds[buf], reinterpret_cast<const char*>(K8) + slice * pbytes, (int)pbytes,
                      reinterpret_cast<const char*>(Vt8) + slice * pbytes, (int)pbytes, walk.sip, ngr, wave);
            walk.advance(any, b);
        } else
            stg.issue(lds[buf], kbase, Nk * RB, vbase, Nk * D, t0 / SG, ngr, wave);
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
        if (32 * t + 31 > L - Nq) {  // wave-uniform: the tile holds a key some column does not see
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int qb = 0; qb < QB; ++qb)
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        s.v[kb][qb][i] = 32 * t + key0 + i + 8 * kb > lim[qb] ? -__builtin_huge_valf() : s.v[kb][qb][i];
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
        const bool ok = l > 1e-10f;
        // row r writes chunk c iff c <= last((s + r) / 32) / C = ((L - Nq + r) / 32) / C: what the combine reads of it
        if (!real[qb] || c > lim[qb] / QMHA_GROUP / out.C) continue;
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

// ---------------------------------------------------------------------------------------
// host: masked_geo's Ragged / Paged geometry of a token-granular call; QB from W = Nq * (H / Hkv); then the combine pass
// ---------------------------------------------------------------------------------------
template <class Geo>
static hipError_t fp8_decode_launch(const Fp8Workspace& w, const float* Qf, float* O, const MaskedCall& c, int chunk_rows, void* scratch,
                                    hipStream_t stream, Geo geo) {
    const int W = c.Nq * (c.H / c.Hkv);
    if (!scratch || W > 32 || chunk_rows < 2 * QMHA_GROUP || chunk_rows % (2 * QMHA_GROUP) != 0 || chunk_rows > c.Nk) return hipErrorInvalidValue;
    const int NC = (c.Nk + chunk_rows - 1) / chunk_rows;
    if ((long long)c.B * c.Hkv * NC > INT_MAX || ((long long)c.Nq * c.d_model / 4 + 255) / 256 * c.B > INT_MAX) return hipErrorInvalidValue;
    const SplitScratch s = split_carve(scratch, c.B, NC, c.Nq, c.H, c.D);
    const DecodeOut out{s.Oc, s.m, s.l, chunk_rows / QMHA_GROUP, NC};
    const dim3 grid(c.B * c.Hkv * NC), block(kWaves * 64);
    const hipError_t e = fp8_cache_d(c.D, [&](auto d) {
        auto go = [&](auto qb) {
            hipLaunchKernelGGL((qmha_fp8_decode_kernel<Geo, decltype(d)::value, decltype(qb)::value>), grid, block, 0, stream, Qf, w.K8, w.Vt8, geo,
                               out, c.lens, c.Hkv, c.d_model, w.q_scale, w.q_scale * w.k_scale * softmax_scale_log2(c.D), w.v_scale);
            return hipGetLastError();
        };
        return W > 16 ? go(std::integral_constant<int, 2>{}) : go(std::integral_constant<int, 1>{});
    });
    if (e != hipSuccess) return e;
    return launch_split_combine(O, Split<Paged>(as_paged(geo), s, out.C, NC), c, 1e-10f, stream);
}

hipError_t launch_fp8_decode(const Fp8Workspace& w, const float* Qf, float* O, const MaskedCall& c, int chunk_rows, void* scratch,
                             hipStream_t stream) {
    if (!c.ragged) return hipErrorInvalidValue;
    return masked_geo(c, [&](auto geo) {
        if constexpr (kRaggedGeo<decltype(geo)>) return fp8_decode_launch(w, Qf, O, c, chunk_rows, scratch, stream, geo);
        else return hipErrorInvalidValue;
    });
}

}  // namespace qmha
