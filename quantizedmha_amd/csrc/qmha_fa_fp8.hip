// qmha_fa_fp8.hip -- the attend kernels of an e4m3 K/V cache (fa_tc_fp8) for gfx950 (MI355X), in a
// translation unit of their own so that every other kernel keeps its bytes.  One template over the geometries of
// qmha_fa_masked.hpp: Grouped (a cache with a host length; G = 1 is the multi-head cache), Varlen (per-sequence lengths),
// Ragged (token-granular lengths) and Paged (a pool of pages behind a block table).  The geometry comes first in the
// template's argument list and D after it.
//
// The contract (include/launchers.h): a cached element is e4m3_rne(clamp(x / scale, -448, 448)); Q converts in registers
// with q_scale; S = (q8 . k8, fp32) * q_scale * k_scale * log2(e) / sqrt(d), masked before the row maximum; the softmax
// is online over a TRUE running maximum m; p = exp2(s - m + 8) is at most 256 < 448 and goes to the matrix core through
// v_cvt_pk_fp8_f32, the row sum l adds the fp32 p, and O = v_scale * o / l, so the bias of 8 cancels.
//
// Work split: the masked fp16 body's.  One wave is a 32-row query group, kWaves of them share the LDS-DMA stages of two
// key tiles, double-buffered; S^T = K Q^T and O^T = V^T P^T both run on v_mfma_f32_16x16x32_fp8_fp8, whose lane
// 16 grp + r16 holds eight bytes (row r16, k = 8 grp .. +7) and whose accumulator map is that of the f16 16x16x32 form:
// kap16, the diagonal select and the epilogue carry over.  What is new:
//   K rows are D bytes.  The sum over d does not care about its order, so k-step (kp, h) gives lane group grp the bytes
//     d = 64 kp + 16 grp + 8 h .. +7 of its K row and of its query: the two k-steps of a kp are then one 16-byte chunk,
//     4 kp + grp, of a row-major row -- one ds_read_b128 feeds two MFMAs, and K stays row-major in memory.  The chunk
//     index is the int8 rows' 4 ks + grp, so kswz16<64> / kswz16<128> keep every 16-lane read group on 16 distinct slots.
//   V^T blocks pair two d-blocks instead (fp8_vt_offset, qmha_kernels.hpp): line 16 mp + r16 of 64 bytes, chunk grp holds
//     the eight key slots of row d = 32 mp + r16 and of row d + 16.  Pairing along the key axis would interleave two
//     32-row groups in memory, and a group is the unit the appends and the pages are made of.  A line is 64 bytes as an f16
//     V^T row is, so vswz16(line) is the conflict-free mask.
//   A stage is 2 * 32 * D bytes of K and as many of V^T: 8 KiB at d = 64, half the fp16 kernel's.
//   The running maximum is formed only when it moves: a lane compares its eight scores of a row with m, and a ballot
//     decides (wave-uniform) whether some row's maximum rises; then the rows' maxima are joined over the four lane groups
//     and m = max(m, row maximum), alpha = exp2(m_old - m) rescales l and o (1 exactly for a row that did not move).  So m
//     is the true running maximum after every tile, with no cross-lane traffic on a tile that leaves it alone.
#include "qmha_fa_masked.hpp"
#include "qmha_fp8.hpp"

#include <utility>

namespace qmha {

template <class Geo, int D>
__global__ __launch_bounds__(kWaves * 64, D > 64 ? 2 : 4) void qmha_fa_fp8_kernel(
    const float* __restrict__ Qf, const uint8_t* __restrict__ K8, const uint8_t* __restrict__ Vt8, float* __restrict__ O, Geo any,
    const int32_t* __restrict__ lens, int H, int d_model, int nqb, float q_scale, float s_log2, float v_scale) {
    // the sequence's geometry: read from device memory where the call has lengths there (workgroup-uniform, before the
    // first barrier or DMA issue), as the fp16 cache and varlen kernels do
    int bh, qb0;
    masked_wg_single(nqb, bh, qb0);
    auto seq = [&]() {
        if constexpr (kRaggedGeo<Geo>) {
            const PackedSeq q = cache_seq(any, lens, bh / H);
            if (q.verdict != 2) {
                if (q.verdict == 1 && qb0 == 0) zero_seq_rows<D>(O, any, q, bh, H, d_model);
                return std::pair<bool, Geo>(false, any);
            }
            return std::pair<bool, Geo>(true, seq_geo(any, q));
        } else if constexpr (std::is_same<Geo, Varlen>::value) {
            const int L = lens[bh / H];
            if (!any.valid(L)) {
                zero_unit_block<D>(O, any, bh, H, d_model, qb0);
                return std::pair<bool, Geo>(false, any);
            }
            return std::pair<bool, Geo>(true, any.of(L));
        } else
            return std::pair<bool, Geo>(true, any);
    }();
    if (!seq.first) return;
    const Geo geo = seq.second;

    asm volatile("" : "+v"(s_log2));  // a VOP3 fma reading an SGPR issues at the slow rate
    constexpr int WAVES = kWaves, SG = kSG;
    constexpr int KP = D / 64;            // 16-byte chunks a lane reads of a K row: two QK k-steps each
    constexpr int DB = D / 16;            // PV d-blocks of 16 rows, read in pairs
    constexpr int RB = D;                 // K row bytes
    constexpr int KBYTES = SG * 32 * RB;  // K per stage
    constexpr int VBYTES = SG * 32 * D;   // V^T per stage
    constexpr int KCH = KBYTES / 16, VCH = VBYTES / 16;
    static_assert(D == 64 || D == 128, "fp8 cache: d in {64, 128}");
    static_assert(KCH % 64 == 0 && VCH % 64 == 0 && (KCH / SG) % 64 == 0 && (VCH / SG) % 64 == 0, "whole KiB LDS-DMA pieces");
    __shared__ __attribute__((aligned(16))) char lds[2][KBYTES + VBYTES];

    const int Nk = geo.nk();
    const int U = geo.units();
    const int b = bh / H, kvh = bh % H;  // bh: the K/V slice (H K/V heads)
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if constexpr (kRaggedGeo<Geo>) {  // its grid follows the host's Nq, U the sequence's length: a workgroup with
        if (qb0 * WAVES >= U) return;  // no active unit leaves before any barrier or DMA issue
    }
    const int u = qb0 * WAVES + wave;
    const bool active = u < U;
    const int qg = geo.group(u), k = geo.head(kvh, u);  // query group, query head
    const int grp = lane >> 4, r16 = lane & 15;
    const int wg_last = geo.last(geo.group(min(qb0 * WAVES + WAVES - 1, U - 1)));  // of the last active wave
    const int nst = wg_last / SG + 1;
    const int my_diag = geo.diag(qg);
    const int my_last = active ? geo.last(qg) : -1;

    // Q into the QK B operand: query 16 qb + r16, bytes d = 64 kp + 16 grp + 8 h .. +7 for k-step 2 kp + h
    fp8x8 qop[2][2 * KP];
#pragma unroll
    for (int qb = 0; qb < 2; ++qb)
#pragma unroll
        for (int ks = 0; ks < 2 * KP; ++ks) {
            float x[8] = {};
            if (active && row_real(geo, qg * QMHA_GROUP + 16 * qb + r16)) {  // a pad lane (Ragged) loads nothing
                const float* qp = Qf + (seq_row0(geo, b) + (size_t)qg * QMHA_GROUP + 16 * qb + r16 - row_shift(geo)) * d_model + (size_t)k * D +
                                  64 * (ks >> 1) + 16 * grp + 8 * (ks & 1);
                const v4f a = *reinterpret_cast<const v4f*>(qp), c = *reinterpret_cast<const v4f*>(qp + 4);
#pragma unroll
                for (int e = 0; e < 4; ++e) x[e] = fp8_prep(a[e], q_scale), x[4 + e] = fp8_prep(c[e], q_scale);
            }
            qop[qb][ks] = fp8_pack8(x);
        }
    v4f o[DB][2];
#pragma unroll
    for (int m = 0; m < DB; ++m) o[m][0] = o[m][1] = v4f{};
    // mb: the running maximum less the bias of 8 (log2 units; x - 8 is monotone, so the maximum of the biased scores);
    // no score is below -1e30.  l: over this lane's keys
    float mb[2] = {-1e30f, -1e30f}, l_run[2] = {0.0f, 0.0f};

    const char* kbase = reinterpret_cast<const char*>(K8 + (size_t)bh * Nk * D);
    const char* vbase = reinterpret_cast<const char*>(Vt8 + (size_t)bh * Nk * D);
    MaskedStager<WAVES, KCH, VCH, KBYTES, VBYTES, SG> stg;
#pragma unroll
    for (int jj = 0; jj < stg.KJ; ++jj) {
        const int idx = (wave + jj * WAVES) * 64 + lane;
        const int row = idx / (RB / 16), cc = (idx % (RB / 16)) ^ kswz16<RB>(row);
        stg.koff[jj] = row * RB + 16 * cc;
    }
#pragma unroll
    for (int jj = 0; jj < stg.VJ; ++jj) {
        const int idx = (wave + jj * WAVES) * 64 + lane;
        const int gq = idx / (2 * D), w = idx % (2 * D);
        const int line = w >> 2, cv = (w & 3) ^ vswz16(line);
        stg.voff[jj] = gq * 32 * D + line * 64 + 16 * cv;
    }
    // Paged: the stage's page slice is the buffer, the stage offset the stage's place in its page
    std::conditional_t<kPagedGeo<Geo>, PageWalk, NoWalk> walk;
    if constexpr (kPagedGeo<Geo>) walk.start(geo, b);
    auto issue = [&](int buf, int st) {
        if constexpr (kPagedGeo<Geo>) {
            walk.take(geo);
            const size_t slice = (size_t)walk.page * H + kvh, pbytes = (size_t)geo.PG * (QMHA_GROUP * D);
            stg.issue(lds[buf], reinterpret_cast<const char*>(K8) + slice * pbytes, (int)pbytes,
                      reinterpret_cast<const char*>(Vt8) + slice * pbytes, (int)pbytes, walk.sip, min(SG, wg_last + 1 - st * SG), wave);
            walk.advance(geo, b);
        } else
            stg.issue(lds[buf], kbase, Nk * RB, vbase, Nk * D, st, min(SG, wg_last + 1 - st * SG), wave);
    };
    // S^T blocks [kb][qb] of tile gi: rows kap16(kb, .) of the K tile against query block qb
    struct S4 {
        v4f v[2][2];
    };
    auto qk = [&](const char* L, int gi) {
        S4 s;
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
            const int krow = gi * 32 + kap16(kb, r16);
            s.v[kb][0] = s.v[kb][1] = v4f{};
#pragma unroll
            for (int kp = 0; kp < KP; ++kp) {
                const v2l kop = *reinterpret_cast<const v2l*>(L + krow * RB + 16 * ((4 * kp + grp) ^ kswz16<RB>(krow)));
#pragma unroll
                for (int h = 0; h < 2; ++h)
#pragma unroll
                    for (int qb = 0; qb < 2; ++qb)
                        s.v[kb][qb] = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(kop[h], qop[qb][2 * kp + h], s.v[kb][qb], 0, 0, 0);
            }
        }
        return s;
    };
    const int key0 = kap16(0, 4 * grp);  // this lane's keys of the tile: key0 + i + 8 kb
    auto tile = [&](const char* L, int gi, S4 s, bool diag) {
        v2l vop[DB / 2];  // V^T rows 32 mp + r16 and + 16, slots 8 grp .. +7 (read before the softmax)
#pragma unroll
        for (int mp = 0; mp < DB / 2; ++mp) {
            const int line = 16 * mp + r16;
            vop[mp] = *reinterpret_cast<const v2l*>(L + KBYTES + gi * 32 * D + line * 64 + 16 * (grp ^ vswz16(line)));
        }
        if (diag) {  // wave-uniform: one select per score, before any use
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int qb = 0; qb < 2; ++qb)
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        s.v[kb][qb][i] = key0 + i + 8 * kb > 16 * qb + r16 ? -__builtin_huge_valf() : s.v[kb][qb][i];
        }
        float sc[2][8], mx[2];
#pragma unroll
        for (int qb = 0; qb < 2; ++qb) {
#pragma unroll
            for (int j = 0; j < 8; ++j) sc[qb][j] = s.v[j >> 2][qb][j & 3] * s_log2;  // masked: -inf
            mx[qb] = fmaxf(fmaxf(fmaxf(sc[qb][0], sc[qb][1]), fmaxf(sc[qb][2], sc[qb][3])),
                           fmaxf(fmaxf(sc[qb][4], sc[qb][5]), fmaxf(sc[qb][6], sc[qb][7])));
        }
        if (__builtin_amdgcn_ballot_w64(mx[0] - 8.0f > mb[0] || mx[1] - 8.0f > mb[1])) {  // wave-uniform: some row's maximum rises
#pragma unroll
            for (int qb = 0; qb < 2; ++qb) {
                float r = mx[qb];  // the query's four lane groups
                r = fmaxf(r, __shfl_xor(r, 16));
                r = fmaxf(r, __shfl_xor(r, 32));
                const float m_b = fmaxf(mb[qb], r - 8.0f);
                const float alpha = __builtin_amdgcn_exp2f(mb[qb] - m_b);  // 1 for a row that stays
                l_run[qb] *= alpha;
#pragma unroll
                for (int m = 0; m < DB; ++m) o[m][qb] *= alpha;
                mb[qb] = m_b;
            }
        }
#pragma unroll
        for (int qb = 0; qb < 2; ++qb) {
            float p[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) p[j] = __builtin_amdgcn_exp2f(sc[qb][j] - mb[qb]);  // <= 2^8; masked: 0
            l_run[qb] += ((p[0] + p[1]) + (p[2] + p[3])) + ((p[4] + p[5]) + (p[6] + p[7]));
            const fp8x8 pop = fp8_pack8(p);
#pragma unroll
            for (int m = 0; m < DB; ++m) o[m][qb] = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(vop[m >> 1][m & 1], pop, o[m][qb], 0, 0, 0);
        }
    };

    issue(0, 0);
    qmha_dma_barrier();
    auto stage = [&](auto BUF, int st) {
        constexpr int buf = decltype(BUF)::value;
        if (st + 1 < nst) issue(buf ^ 1, st + 1);
        const int t0 = st * SG;
        if (t0 <= my_last) {  // wave-uniform
            const char* L = lds[buf];
#pragma unroll
            for (int gi = 0; gi < SG; ++gi) {
                const int t = t0 + gi;
                if (t <= my_last) tile(L, gi, qk(L, gi), t == my_diag);
                __builtin_amdgcn_sched_barrier(0);  // one tile's registers at a time
            }
        }
        qmha_dma_barrier();
    };
    int st = 0;
    for (; st + 2 <= nst; st += 2) {
        stage(std::integral_constant<int, 0>{}, st);
        stage(std::integral_constant<int, 1>{}, st + 1);
    }
    if (st < nst) stage(std::integral_constant<int, 0>{}, st);
    if (active) {
#pragma unroll
        for (int qb = 0; qb < 2; ++qb) {
            float l = l_run[qb];
            l += __shfl_xor(l, 16);
            l += __shfl_xor(l, 32);
            const bool ok = l > 1e-10f;  // the fp16 epilogue's guard
            float* orow = O + (seq_row0(geo, b) + (size_t)qg * QMHA_GROUP + 16 * qb + r16 - row_shift(geo)) * d_model + (size_t)k * D + 4 * grp;
            if (row_real(geo, qg * QMHA_GROUP + 16 * qb + r16)) {  // a pad lane stores nothing
#pragma unroll
                for (int m = 0; m < DB; ++m) {
                    v4f w;
#pragma unroll
                    for (int j = 0; j < 4; ++j) w[j] = ok ? v_scale * (o[m][qb][j] / l) : 0.0f;
                    *reinterpret_cast<v4f*>(orow + 16 * m) = w;
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------------------
// host: masked_geo's geometry of a cache call; the multi-head cache with a host length (Rect) runs Grouped at G = 1,
// whose unit map is Rect's
// ---------------------------------------------------------------------------------------
template <class Geo>
static hipError_t fa_fp8_launch(const Fp8Workspace& w, const float* Qf, float* O, const MaskedCall& c, hipStream_t stream, Geo geo) {
    const int nqb = masked_nqb(grid_units(geo));
    const dim3 grid(c.B * c.Hkv * nqb), block(kWaves * 64);
    return fp8_cache_d(c.D, [&](auto d) {
        hipLaunchKernelGGL((qmha_fa_fp8_kernel<Geo, decltype(d)::value>), grid, block, 0, stream, Qf, w.K8, w.Vt8, O, geo, c.lens, c.Hkv,
                           c.d_model, nqb, w.q_scale, w.q_scale * w.k_scale * softmax_scale_log2(c.D), w.v_scale);
        return hipGetLastError();
    });
}

hipError_t launch_fa_masked(const Fp8Workspace& w, const float* Qf, float* O, const MaskedCall& c, hipStream_t stream) {
    if (!c.lens && c.len < 0) return hipErrorInvalidValue;  // a K/V cache variant: no call of its own
    return masked_geo(c, [&](auto geo) {
        using G = decltype(geo);
        if constexpr (std::is_same<G, SquareCausal>::value) return hipErrorInvalidValue;
        else if constexpr (std::is_same<G, Rect>::value) return fa_fp8_launch(w, Qf, O, c, stream, Grouped(geo, 1));
        else return fa_fp8_launch(w, Qf, O, c, stream, geo);
    });
}

}  // namespace qmha
