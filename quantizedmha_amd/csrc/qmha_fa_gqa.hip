// qmha_fa_gqa.hip -- grouped-query attention (GQA / MQA) for gfx950 (MI355X): the main
// kernels of the int8 and fp16 fused paths when h query heads share h_kv < h key/value heads, G = h / h_kv.
//
// These are the Rect kernels of qmha_fa_masked.hip with a grouped geometry.  Q and O are [B, Nq, h * D]; K and V
// are [B, Nk, h_kv * D], and the pre-pass (qmha_prepass.hip) runs unchanged over them with H = h_kv, so the
// workspace holds B * h_kv slices of Nk rows and the quantisation groups are per (K/V head, 32 rows).
// What is as in qmha_fa_masked.hip: one wave = one 32-row query group of one query head, a workgroup of 4 waves
// shares the LDS-DMA K/V staging (stages of 2 key tiles, double-buffered), the tile bodies, the anchors / lazy
// base and the epilogues -- the arithmetic and the tile order of a wave are those of the Rect instance, so a
// query head's result is that of the multi-head call on K / V expanded G times, bit for bit.
// What differs:
//   K/V slice.  The K/V bases, the three buffer-descriptor extents and the sK / sV index use the K/V slice
//     b * h_kv + k / G of query head k; query rows and O rows keep d_model = h * D and column k * D.
//   Units.  One K/V slice serves U = G * Gq units: unit u = qg * G + j is query group qg of query head
//     kvh * G + j.  A workgroup holds four consecutive units (nqb = ceil(U / 4)); a wave is active when u < U;
//     diag and last take qg = u / G.  qg is non-decreasing in u, so the workgroup's last tile is that of its last
//     active unit.  With G = 4 a workgroup is the four heads of one query group: one shared diagonal, no wave
//     idle under the mask (decode, Nq = 32: four active waves per workgroup where the Rect kernel has one).
//     G is a run-time, wave-uniform argument (any G >= 2).
//   Grid.  B * h_kv * masked_pairs(nqb) for int8 (mirrored unit-block pairs), B * h_kv * nqb for fp16 (heaviest
//     first); xcd_remap keeps the workgroups of one K/V slice on one XCD, so the G heads re-read K/V from its L2.
// Out of range by construction, as for Rect: K/V reads go through buffer descriptors of exactly the (b, kvh)
// slice and a stage issues whole tiles t <= Gk - 1 only; sK / sV are read at t <= Gk - 1 of slice bkv * Gk;
// Q and O rows are touched by active waves only (qg < Gq, query head < h).
//
// Duplicated from qmha_fa_masked.hip (which stays textually as it is, so that every kernel it holds keeps its
// instruction bytes): the stager, the launch-index maps and both kernel bodies without the dumping branches.
#include "qmha_common.hpp"
#include "qmha_kernels.hpp"

#include <type_traits>

namespace qmha {

constexpr float kGqaLazySumCap = 4096.0f;  // the fp16 lazy base's cap
constexpr int kGqaWaves = 4, kGqaSG = 2;

// The geometry of a grouped launch: Rect's rows and diagonal, and G query heads per K/V head.
// causal: bottom-right aligned, diag_off = Gk - Gq; else diag_off = Gk, a diagonal no tile reaches.
struct Grouped {
    int Nq, Nk, diag_off, G;
    Grouped(int nq, int nk, bool causal, int g)
        : Nq(nq), Nk(nk), diag_off(nk / QMHA_GROUP - (causal ? nq / QMHA_GROUP : 0)), G(g) {}
    // the causal geometry of a K/V cache: Nk = cap, the diagonal of the last query group on tile
    // len / 32 - 1, so no tile at or beyond len / 32 is staged or computed.  nq <= len <= cap.
    static Grouped cached(int nq, int cap, int len, int g) {
        Grouped r(nq, cap, false, g);
        r.diag_off = (len - nq) / QMHA_GROUP;
        return r;
    }
    __device__ int gq() const { return Nq / QMHA_GROUP; }
    __device__ int gk() const { return Nk / QMHA_GROUP; }
    __device__ int units() const { return G * gq(); }
    __device__ int diag(int qg) const { return qg + diag_off; }  // >= Gk: none
    __device__ int last(int qg) const { return min(qg + diag_off, gk() - 1); }
};

namespace {

// Launch index -> (K/V slice, unit-block pair) and (K/V slice, unit block): masked_wg / masked_wg_single of
// qmha_fa_masked.hip over unit blocks
__host__ __device__ constexpr int gqa_pairs(int nqb) { return (nqb + 1) / 2; }
__device__ __forceinline__ void gqa_wg_single(int nqb, int& bkv, int& qb) {
    const int wg = xcd_remap(blockIdx.x, gridDim.x);
    bkv = wg / nqb;
    qb = nqb - 1 - wg % nqb;
}
__device__ __forceinline__ void gqa_wg(int nqb, int& bkv, int& pi) {
    const int wg = xcd_remap(blockIdx.x, gridDim.x);
    bkv = wg / gqa_pairs(nqb);
    pi = wg % gqa_pairs(nqb);
}

// K/V staging (MaskedStager of qmha_fa_masked.hip)
template <int WAVES, int KCH, int VCH, int KBYTES, int VBYTES, int SG>
struct GqaStager {
    static constexpr int KJ = (KCH / 64 + WAVES - 1) / WAVES, VJ = (VCH / 64 + WAVES - 1) / WAVES;
    int koff[KJ], voff[VJ];
    // ngr: tiles of the stage to bring in (1..SG, wave-uniform)
    __device__ __forceinline__ void issue(char* L, const char* kbase, int knrec, const char* vbase, int vnrec, int st,
                                          int ngr, int wave) const {
#pragma unroll
        for (int jj = 0; jj < KJ; ++jj) {
            const int inst = wave + jj * WAVES;
            if (inst < KCH / 64 && inst * 64 < ngr * (KCH / SG))
                buffer_load_lds16(kbase, knrec, (lptr_t)(L + inst * 1024), koff[jj], st * KBYTES);
        }
#pragma unroll
        for (int jj = 0; jj < VJ; ++jj) {
            const int inst = wave + jj * WAVES;
            if (inst < VCH / 64 && inst * 64 < ngr * (VCH / SG))
                buffer_load_lds16(vbase, vnrec, (lptr_t)(L + KBYTES + inst * 1024), voff[jj], st * VBYTES);
        }
    }
};

}  // namespace

// ---------------------------------------------------------------------------------------
// int8 (fa_tc_int8_b contract): qmha_fa_int8_masked_kernel<D, Rect> over units
// ---------------------------------------------------------------------------------------
template <int D>
__global__ __launch_bounds__(kGqaWaves * 64, D > 64 ? 2 : 4) void qmha_fa_int8_gqa_kernel(
    const float* __restrict__ Qf, const int8_t* __restrict__ Ki, const _Float16* __restrict__ Vh,
    const float* __restrict__ sK, const float* __restrict__ sV, float* __restrict__ O, Grouped geo, int Hkv, int d_model,
    int nqb, float c_log2) {
    constexpr int WAVES = kGqaWaves, SG = kGqaSG;
    constexpr int KS = D / 32;               // i8 MFMA k-steps (QK) and d-blocks (PV)
    constexpr int KBYTES = SG * 32 * D;      // K int8 per stage
    constexpr int VBYTES = SG * 32 * D * 2;  // V f16 per stage
    constexpr int KCH = KBYTES / 16, VCH = VBYTES / 16;
    static_assert(D == 32 || D == 64 || D == 128, "grouped int8: d in {32, 64, 128}");
    static_assert(KCH % 64 == 0 && VCH % 64 == 0 && (KCH / SG) % 64 == 0, "whole KiB LDS-DMA pieces");
    __shared__ __attribute__((aligned(16))) char lds[2][KBYTES + VBYTES];

    const int Nq = geo.Nq, Nk = geo.Nk;
    const int Gk = geo.gk(), U = geo.units();
    int bkv, pi;
    gqa_wg(nqb, bkv, pi);
    const int b = bkv / Hkv, kvh = bkv % Hkv;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int half = lane >> 5, col = lane & 31;
#pragma nounroll
    for (int pass = 0; pass < 2; ++pass) {  // the pair's large unit block, then its mirror (uniform)
    const int qb = pass == 0 ? nqb - 1 - pi : pi;
    if (pass == 1 && pi == nqb - 1 - pi) break;  // odd nqb: the middle unit block has no partner
    const int u = qb * WAVES + wave;
    const bool active = u < U;  // wave-uniform; an inactive wave still stages and syncs
    const int qg = (int)((unsigned)u / (unsigned)geo.G);               // query group
    const int k = kvh * geo.G + (int)((unsigned)u % (unsigned)geo.G);  // query head
    // the workgroup's last tile: that of its last active unit
    const int wg_last = geo.last((int)((unsigned)min(qb * WAVES + WAVES - 1, U - 1) / (unsigned)geo.G));
    const int nst = wg_last / SG + 1;
    const int my_diag = geo.diag(qg);                // this wave's diagonal tile
    const int my_last = active ? geo.last(qg) : -1;  // this wave computes tiles t <= my_last

    // in-register Q quantisation (fa_tc_int8_b.cu:33-152) into the Q^T operand: lane (col, half) holds
    // bytes [32 s + 16 half, +16) of query row col for every k-step s
    v4i qop[KS];
    float cq = 0.0f;
    if (active) {
        const float* qrow = Qf + ((size_t)b * Nq + (size_t)qg * QMHA_GROUP + col) * d_model + (size_t)k * D;
        v4f x[KS][4];
        float amax = 0.0f;
#pragma unroll
        for (int s = 0; s < KS; ++s)
#pragma unroll
            for (int c4 = 0; c4 < 4; ++c4) {
                x[s][c4] = *reinterpret_cast<const v4f*>(qrow + 32 * s + 16 * half + 4 * c4);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    x[s][c4][e] = nan_to_zero(x[s][c4][e]);
                    amax = fmaxf(amax, fabsf(x[s][c4][e]));
                }
            }
        const float sq = qmha_scale_from_absmax(wave_max64(amax));
        const float inv = 1.0f / sq;
#pragma unroll
        for (int s = 0; s < KS; ++s)
#pragma unroll
            for (int c4 = 0; c4 < 4; ++c4) {
                uint32_t w = 0;
#pragma unroll
                for (int e = 0; e < 4; ++e) w |= ((uint32_t)(uint8_t)qmha_quant_i8(x[s][c4][e], inv)) << (8 * e);
                qop[s][c4] = (int)w;
            }
        cq = sq * c_log2;
    } else {
#pragma unroll
        for (int s = 0; s < KS; ++s) qop[s] = v4i{0, 0, 0, 0};
    }
    v16f o[KS];
#pragma unroll
    for (int m = 0; m < KS; ++m) o[m] = v16f{};
    float m_run = 0.0f;   // m0 = 0 (fa_tc_int8_b.cu:402), log2 units
    float l_run = 0.0f;   // anchored: l * 2^(m - anchor), over this lane's half of the keys
    float anchor = 0.0f;  // o = O * 2^(m - anchor), anchor <= m

    const char* kbase = reinterpret_cast<const char*>(Ki + (size_t)bkv * Nk * D);
    const char* vbase = reinterpret_cast<const char*>(Vh + (size_t)bkv * Nk * D);
    const float* skb = sK + (size_t)bkv * Gk;
    const float* svb = sV + (size_t)bkv * Gk;

    GqaStager<WAVES, KCH, VCH, KBYTES, VBYTES, SG> stg;
#pragma unroll
    for (int jj = 0; jj < stg.KJ; ++jj) {
        const int idx = (wave + jj * WAVES) * 64 + lane;
        const int row = idx / (D / 16), cc = swz_src<D>(row, idx % (D / 16));
        stg.koff[jj] = row * D + 16 * cc;
    }
#pragma unroll
    for (int jj = 0; jj < stg.VJ; ++jj) {
        const int idx = (wave + jj * WAVES) * 64 + lane;
        const int grp = idx / (4 * D), w = idx % (4 * D);
        const int d = w >> 2, cv = swz_src<64>(d, w & 3);
        stg.voff[jj] = grp * 64 * D + d * 64 + 16 * cv;
    }
    auto issue = [&](int buf, int st) {
        stg.issue(lds[buf], kbase, Nk * D, vbase, Nk * D * 2, st, min(SG, wg_last + 1 - st * SG), wave);
    };

    // S^T = K Q^T of tile gi of the stage in LDS (int32, exact)
    auto qk = [&](const char* L, int gi) {
        const int krow = gi * 32 + col;
        v16i s = v16i{};
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const v4i kop = *reinterpret_cast<const v4i*>(L + krow * D + 16 * swz_pos<D>(krow, 2 * ks + half));
            s = __builtin_amdgcn_mfma_i32_32x32x32_i8(kop, qop[ks], s, 0, 0, 0);
        }
        return s;
    };
    const int mask_col = col - 4 * half;  // key acc_row(r, half) > col  <=>  acc_row(r, 0) > mask_col

    // one tile: online softmax (fa_tc_int8_b.cu:281-346), P quantisation (:359), P@V (:366-371);
    // diag: the diagonal tile
    auto tile = [&](const char* L, int gi, int t, const v16i& s, bool diag) {
        const float skt = skb[t], svt = svb[t];
        const float c = cq * skt;  // sQ*sK*log2(e)/sqrt(d) > 0
        float sf[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) sf[r] = (float)s[r];
        if (diag) {  // wave-uniform: one select per score, before the row max
#pragma unroll
            for (int r = 0; r < 16; ++r) sf[r] = acc_row(r, 0) > mask_col ? -__builtin_huge_valf() : sf[r];
        }
        float mx = fmaxf(fmaxf(sf[0], sf[1]), sf[2]);
#pragma unroll
        for (int r = 3; r < 15; r += 2) mx = fmaxf(fmaxf(mx, sf[r]), sf[r + 1]);
        mx = half_swap_max(fmaxf(mx, sf[15]));  // finite: key 0 of the tile is never masked
        const float m_new = fmaxf(m_run, mx * c);
        // tile max of p = exp(row max - m), then the max over the 32 query rows (:359)
        const float pmax = half_max32_nonneg(__builtin_amdgcn_exp2f(fmaf(mx, c, -m_new)));
        const float sp = fmaxf(div127_fast(pmax), 1e-8f);  // sP = max(absmax/127, 1e-8)
        const float invp = rcp_fast(sp);                   // 1/sP
        float p[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) p[r] = __builtin_amdgcn_exp2f(fmaf(sf[r], c, -m_new));  // masked: exp2(-inf) = 0
        // Pi = rint(p/sP) (0..127), carried as the f16 subnormal Pi * 2^-24 (see qmha_fa_masked.hip)
        v8h pop[2];
#pragma unroll
        for (int r = 0; r < 16; r += 2) {
            const float t0 = fmaf(p[r], invp, QMHA_MAGIC_RNE), t1 = fmaf(p[r + 1], invp, QMHA_MAGIC_RNE);
            const v2h h2 = __builtin_bit_cast(v2h, __builtin_amdgcn_perm(__float_as_uint(t1), __float_as_uint(t0), 0x05040100u));
            pop[r >> 3][r & 7] = h2[0];
            pop[r >> 3][(r & 7) + 1] = h2[1];
        }
        // row sum of the unquantised p (:336) over this lane's 16 keys; the two halves of l are joined once,
        // in the epilogue (every factor l takes below is the same in both halves of a row)
        const float rs = tree_sum16(p);
        // anchored running state, as qmha_fa_int8_kernel: o += T*sP*sV*2^(m_t - anchor),
        // l_run += rowsum*2^(m_t - anchor); re-anchor before the shift is formed
        if (__builtin_amdgcn_ballot_w64(m_new - anchor > 48.0f)) {
            const float f = __builtin_amdgcn_exp2f(anchor - m_new);
#pragma unroll
            for (int m = 0; m < KS; ++m) o[m] *= f;
            l_run *= f;
            anchor = m_new;
        }
        const float e = __builtin_amdgcn_exp2f(m_new - anchor);
        l_run = fmaf(rs, e, l_run);
        m_run = m_new;
        const float scale = (sp * 16777216.0f) * svt * e;  // 2^24: the P entries are Pi * 2^-24
#pragma unroll
        for (int m = 0; m < KS; ++m) {
            const int d = 32 * m + col;
            const char* vr = L + KBYTES + gi * 64 * D + d * 64;
            v16f acc = v16f{};
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                const v8h vop = *reinterpret_cast<const v8h*>(vr + 16 * swz_pos<64>(d, 2 * ks + half));
                acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(vop, pop[ks], acc, 0, 0, 0);
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) o[m][r] = fmaf(acc[r], scale, o[m][r]);
        }
    };

    issue(0, 0);
    qmha_dma_barrier();  // waits vmcnt(0): stage 0 has landed
    auto stage = [&](auto BUF, int st) {
        constexpr int buf = decltype(BUF)::value;
        if (st + 1 < nst) issue(buf ^ 1, st + 1);  // buf^1 was released by the previous barrier
        const int t0 = st * SG;
        if (t0 <= my_last) {  // wave-uniform
            const char* L = lds[buf];
#pragma unroll
            for (int gi = 0; gi < SG; ++gi) {
                const int t = t0 + gi;
                if (t <= my_last) tile(L, gi, t, qk(L, gi), t == my_diag);
                __builtin_amdgcn_sched_barrier(0);  // one tile's registers at a time
            }
        }
        qmha_dma_barrier();  // vmcnt(0) + barrier: stage st+1 landed, stage st released
    };
    int st = 0;
    for (; st + 2 <= nst; st += 2) {
        stage(std::integral_constant<int, 0>{}, st);
        stage(std::integral_constant<int, 1>{}, st + 1);
    }
    if (st < nst) stage(std::integral_constant<int, 0>{}, st);

    // ---- epilogue (fa_tc_int8_b.cu:540-578): out = O / l, 0 if l <= 1e-20 -----------------
    if (active) {
        const float unanchor = __builtin_amdgcn_exp2f(anchor - m_run);  // 2^(anchor - m)
        const float l = half_swap_add(l_run) * unanchor;
        const bool ok = l > 1e-20f;
        float* orow = O + ((size_t)b * Nq + (size_t)qg * QMHA_GROUP + col) * d_model + (size_t)k * D + 4 * half;
#pragma unroll
        for (int m = 0; m < KS; ++m)
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) {
                v4f w;
#pragma unroll
                for (int jj = 0; jj < 4; ++jj) w[jj] = ok ? (o[m][4 * g4 + jj] * unanchor) / l : 0.0f;
                *reinterpret_cast<v4f*>(orow + 32 * m + 8 * g4) = w;
            }
    }
    }  // pass: the last stage's barrier has released both LDS buffers
}

// ---------------------------------------------------------------------------------------
// fp16 (fa_tc_v1a contract): qmha_fa_f16_masked_kernel<D, Rect> over units
// ---------------------------------------------------------------------------------------
template <int D>
__global__ __launch_bounds__(kGqaWaves * 64, D > 64 ? 2 : 4) void qmha_fa_f16_gqa_kernel(
    const float* __restrict__ Qf, const _Float16* __restrict__ Kh, const _Float16* __restrict__ Vt,
    float* __restrict__ O, Grouped geo, int Hkv, int d_model, int nqb, float c_log2) {
    QMHA_ENABLE_AGPR_MFMA();
    asm volatile("" : "+v"(c_log2));  // a VOP3 fma reading an SGPR issues at the slow rate
    constexpr int WAVES = kGqaWaves, SG = kGqaSG;
    constexpr int KS = D / 32;            // QK k-steps (K = 32)
    constexpr int DB = D / 16;            // PV d-blocks of 16 rows
    constexpr int RB = 2 * D;             // K row bytes
    constexpr int KBYTES = SG * 32 * RB;  // K per stage
    constexpr int VBYTES = SG * 32 * D * 2;
    constexpr int KCH = KBYTES / 16, VCH = VBYTES / 16;
    static_assert(D == 64 || D == 128, "grouped fp16: d in {64, 128}");
    static_assert(KCH % 64 == 0 && VCH % 64 == 0 && (KCH / SG) % 64 == 0, "whole KiB LDS-DMA pieces");
    __shared__ __attribute__((aligned(16))) char lds[2][KBYTES + VBYTES];

    const int Nq = geo.Nq, Nk = geo.Nk;
    const int U = geo.units();
    int bkv, qb0;
    gqa_wg_single(nqb, bkv, qb0);
    const int b = bkv / Hkv, kvh = bkv % Hkv;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int u = qb0 * WAVES + wave;
    const bool active = u < U;
    const int qg = (int)((unsigned)u / (unsigned)geo.G);               // query group
    const int k = kvh * geo.G + (int)((unsigned)u % (unsigned)geo.G);  // query head
    const int grp = lane >> 4, r16 = lane & 15;
    // of the last active unit
    const int wg_last = geo.last((int)((unsigned)min(qb0 * WAVES + WAVES - 1, U - 1) / (unsigned)geo.G));
    const int nst = wg_last / SG + 1;
    const int my_diag = geo.diag(qg);  // this wave's diagonal tile
    const int my_last = active ? geo.last(qg) : -1;

    // Q converted in-kernel (RNE) into the QK B operand: query 16 qb + r16, d = 32 ks + 8 grp .. +7
    v8h qop[2][KS];
#pragma unroll
    for (int qb = 0; qb < 2; ++qb)
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            if (active) {
                const float* qp = Qf + ((size_t)b * Nq + (size_t)qg * QMHA_GROUP + 16 * qb + r16) * d_model + (size_t)k * D +
                                  32 * ks + 8 * grp;
                const v4f a = *reinterpret_cast<const v4f*>(qp), c = *reinterpret_cast<const v4f*>(qp + 4);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    qop[qb][ks][e] = (_Float16)a[e];
                    qop[qb][ks][4 + e] = (_Float16)c[e];
                }
            } else {
#pragma unroll
                for (int e = 0; e < 8; ++e) qop[qb][ks][e] = (_Float16)0.0f;
            }
        }
    v4f o[DB][2];
#pragma unroll
    for (int m = 0; m < DB; ++m) o[m][0] = o[m][1] = v4f{};
    float m_run[2] = {0.0f, 0.0f}, l_run[2] = {0.0f, 0.0f};  // m0 = 0 (fa_tc_v1a.cu:290); l over this lane's keys

    const char* kbase = reinterpret_cast<const char*>(Kh + (size_t)bkv * Nk * D);
    const char* vbase = reinterpret_cast<const char*>(Vt + (size_t)bkv * Nk * D);

    GqaStager<WAVES, KCH, VCH, KBYTES, VBYTES, SG> stg;
#pragma unroll
    for (int jj = 0; jj < stg.KJ; ++jj) {
        const int idx = (wave + jj * WAVES) * 64 + lane;
        const int row = idx / (RB / 16), cc = (idx % (RB / 16)) ^ kswz16<RB>(row);
        stg.koff[jj] = row * RB + 16 * cc;
    }
#pragma unroll
    for (int jj = 0; jj < stg.VJ; ++jj) {
        const int idx = (wave + jj * WAVES) * 64 + lane;
        const int gq = idx / (4 * D), w = idx % (4 * D);
        const int d = w >> 2, cv = (w & 3) ^ vswz16(d);
        stg.voff[jj] = gq * 64 * D + d * 64 + 16 * cv;
    }
    auto issue = [&](int buf, int st) {
        stg.issue(lds[buf], kbase, Nk * RB, vbase, Nk * D * 2, st, min(SG, wg_last + 1 - st * SG), wave);
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
            for (int ks = 0; ks < KS; ++ks) {
                const v8h kop = *reinterpret_cast<const v8h*>(L + krow * RB + 16 * ((4 * ks + grp) ^ kswz16<RB>(krow)));
#pragma unroll
                for (int qb = 0; qb < 2; ++qb) s.v[kb][qb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kop, qop[qb][ks], s.v[kb][qb], 0, 0, 0);
            }
        }
        return s;
    };
    const int key0 = kap16(0, 4 * grp);  // this lane's keys of the tile: key0 + i + 8 kb
    // online softmax of one tile (fa_tc_v1a.cu:101-220) and O += P V, the lazy base as
    // qmha_fa_f16_v3_kernel; diag: the diagonal tile
    auto tile = [&](const char* L, int gi, S4 s, bool diag) {
        v8h vop[DB];  // V^T rows 16 m + r16, slots 8 grp .. +7 (read before the softmax)
#pragma unroll
        for (int m = 0; m < DB; ++m) {
            const int d = 16 * m + r16;
            vop[m] = *reinterpret_cast<const v8h*>(L + KBYTES + gi * 64 * D + d * 64 + 16 * (grp ^ vswz16(d)));
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
        float p[2][8];
        float ts[2];
        auto softmax_p = [&]() {
#pragma unroll
            for (int qb = 0; qb < 2; ++qb) {
#pragma unroll
                for (int j = 0; j < 8; ++j)
                    p[qb][j] = __builtin_amdgcn_exp2f(fmaf(s.v[j >> 2][qb][j & 3], c_log2, -m_run[qb]));  // masked: 0
                float q0 = p[qb][0] + p[qb][1], q1 = p[qb][2] + p[qb][3], q2 = p[qb][4] + p[qb][5], q3 = p[qb][6] + p[qb][7];
                ts[qb] = (q0 + q1) + (q2 + q3);
            }
        };
        softmax_p();
        const uint64_t over0 = __builtin_amdgcn_ballot_w64(ts[0] > kGqaLazySumCap);
        const uint64_t over1 = __builtin_amdgcn_ballot_w64(ts[1] > kGqaLazySumCap);
        if (over0 | over1) {  // rare (wave-uniform): rebase the queries with a key quarter above the cap
#pragma unroll
            for (int qb = 0; qb < 2; ++qb) {
                const uint64_t over = qb ? over1 : over0;
                float mx = fmaxf(fmaxf(s.v[0][qb][0], s.v[0][qb][1]), fmaxf(s.v[0][qb][2], s.v[0][qb][3]));
                mx = fmaxf(mx, fmaxf(fmaxf(s.v[1][qb][0], s.v[1][qb][1]), fmaxf(s.v[1][qb][2], s.v[1][qb][3])));
                mx = fmaxf(mx, __shfl_xor(mx, 16));  // the query's four lane groups (key 0 is never masked: finite)
                mx = fmaxf(mx, __shfl_xor(mx, 32));
                const uint32_t q16 = (uint32_t)(over | (over >> 32));
                const uint32_t rows = (q16 | (q16 >> 16)) & 0xffffu;
                const float m_b = ((rows >> r16) & 1u) ? mx * c_log2 : m_run[qb];
                const float alpha = __builtin_amdgcn_exp2f(m_run[qb] - m_b);
                l_run[qb] *= alpha;
#pragma unroll
                for (int m = 0; m < DB; ++m) o[m][qb] *= alpha;
                m_run[qb] = m_b;
            }
            softmax_p();
        }
#pragma unroll
        for (int qb = 0; qb < 2; ++qb) {
            l_run[qb] += ts[qb];  // :198 (alpha folded into the rebase above)
            v8h pop;
#pragma unroll
            for (int j = 0; j < 8; j += 2) {
                const v2h h2 = __builtin_convertvector((v2f{p[qb][j], p[qb][j + 1]}), v2h);  // __float2half (RNE), :174
                pop[j] = h2[0];
                pop[j + 1] = h2[1];
            }
#pragma unroll
            for (int m = 0; m < DB; ++m) o[m][qb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vop[m], pop, o[m][qb], 0, 0, 0);
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
            const bool ok = l > 1e-10f;  // fa_tc_v1a.cu:384-388
            float* orow = O + ((size_t)b * Nq + (size_t)qg * QMHA_GROUP + 16 * qb + r16) * d_model + (size_t)k * D + 4 * grp;
#pragma unroll
            for (int m = 0; m < DB; ++m) {
                v4f w;
#pragma unroll
                for (int j = 0; j < 4; ++j) w[j] = ok ? o[m][qb][j] / l : 0.0f;
                *reinterpret_cast<v4f*>(orow + 16 * m) = w;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------
// host launchers
// ---------------------------------------------------------------------------------------
namespace {

bool gqa_rows_ok(int Nq, int Nk) {
    return Nq >= QMHA_GROUP && Nk >= QMHA_GROUP && Nq % QMHA_GROUP == 0 && Nk % QMHA_GROUP == 0;
}
bool gqa_heads_ok(int B, int H, int Hkv, int D, int d_model) {
    return B >= 1 && Hkv >= 1 && Hkv < H && H % Hkv == 0 && d_model == H * D;
}
// a call of its own: the causal mask is bottom-right aligned over Nk >= Nq rows
bool gqa_shape_ok(int Nq, int Nk, bool causal) { return gqa_rows_ok(Nq, Nk) && !(causal && Nk < Nq); }
// a cache of `cap` rows of which `len` are valid: causal Nq <= len <= cap; else every row attends all cap rows
bool gqa_cached_ok(int Nq, int cap, int len, bool causal) {
    if (!gqa_rows_ok(Nq, cap) || len % QMHA_GROUP != 0) return false;
    return causal ? Nq <= len && len <= cap : len == cap;
}
int gqa_nqb(int Nq, int G) { return (G * (Nq / QMHA_GROUP) + kGqaWaves - 1) / kGqaWaves; }  // unit blocks per K/V slice

hipError_t fa_int8_gqa_launch(const Int8Workspace& w, const float* Qf, float* O, int B, Grouped geo, int Hkv, int D, int d_model,
                              hipStream_t stream) {
    const int nqb = gqa_nqb(geo.Nq, geo.G);
    auto launch = [&](auto d) {
        hipLaunchKernelGGL((qmha_fa_int8_gqa_kernel<decltype(d)::value>), dim3(B * Hkv * gqa_pairs(nqb)), dim3(kGqaWaves * 64), 0,
                           stream, Qf, w.Ki, w.Vh, w.sK, w.sV, O, geo, Hkv, d_model, nqb, softmax_scale_log2(D));
        return hipGetLastError();
    };
    switch (D) {
        case 32: return launch(std::integral_constant<int, 32>{});
        case 64: return launch(std::integral_constant<int, 64>{});
        case 128: return launch(std::integral_constant<int, 128>{});
        default: return hipErrorInvalidValue;
    }
}

hipError_t fa_f16_gqa_launch(const F16Workspace& w, const float* Qf, float* O, int B, Grouped geo, int Hkv, int D, int d_model,
                             hipStream_t stream) {
    const int nqb = gqa_nqb(geo.Nq, geo.G);
    auto launch = [&](auto d) {
        hipLaunchKernelGGL((qmha_fa_f16_gqa_kernel<decltype(d)::value>), dim3(B * Hkv * nqb), dim3(kGqaWaves * 64), 0, stream, Qf,
                           w.Kh, w.Vt, O, geo, Hkv, d_model, nqb, softmax_scale_log2(D));
        return hipGetLastError();
    };
    switch (D) {
        case 64: return launch(std::integral_constant<int, 64>{});
        case 128: return launch(std::integral_constant<int, 128>{});
        default: return hipErrorInvalidValue;
    }
}

}  // namespace

hipError_t launch_fa_int8_gqa_main(const Int8Workspace& w, const float* Qf, float* O, int B, int Nq, int Nk, int H, int Hkv,
                                   int D, int d_model, bool causal, hipStream_t stream) {
    if (!gqa_heads_ok(B, H, Hkv, D, d_model) || !gqa_shape_ok(Nq, Nk, causal)) return hipErrorInvalidValue;
    return fa_int8_gqa_launch(w, Qf, O, B, Grouped(Nq, Nk, causal, H / Hkv), Hkv, D, d_model, stream);
}

hipError_t launch_fa_f16_gqa_main(const F16Workspace& w, const float* Qf, float* O, int B, int Nq, int Nk, int H, int Hkv,
                                  int D, int d_model, bool causal, hipStream_t stream) {
    if (!gqa_heads_ok(B, H, Hkv, D, d_model) || !gqa_shape_ok(Nq, Nk, causal)) return hipErrorInvalidValue;
    return fa_f16_gqa_launch(w, Qf, O, B, Grouped(Nq, Nk, causal, H / Hkv), Hkv, D, d_model, stream);
}

hipError_t launch_fa_int8_gqa_cached(const Int8Workspace& w, const float* Qf, float* O, int B, int Nq, int cap, int len, int H,
                                     int Hkv, int D, int d_model, bool causal, hipStream_t stream) {
    if (!gqa_heads_ok(B, H, Hkv, D, d_model) || !gqa_cached_ok(Nq, cap, len, causal)) return hipErrorInvalidValue;
    const int G = H / Hkv;
    return fa_int8_gqa_launch(w, Qf, O, B, causal ? Grouped::cached(Nq, cap, len, G) : Grouped(Nq, cap, false, G), Hkv, D,
                              d_model, stream);
}

hipError_t launch_fa_f16_gqa_cached(const F16Workspace& w, const float* Qf, float* O, int B, int Nq, int cap, int len, int H,
                                    int Hkv, int D, int d_model, bool causal, hipStream_t stream) {
    if (!gqa_heads_ok(B, H, Hkv, D, d_model) || !gqa_cached_ok(Nq, cap, len, causal)) return hipErrorInvalidValue;
    const int G = H / Hkv;
    return fa_f16_gqa_launch(w, Qf, O, B, causal ? Grouped::cached(Nq, cap, len, G) : Grouped(Nq, cap, false, G), Hkv, D,
                             d_model, stream);
}

}  // namespace qmha
