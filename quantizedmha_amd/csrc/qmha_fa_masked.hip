// qmha_fa_masked.hip -- the main kernels of the int8 and fp16 fused attention paths that visit a masked or
// partial set of key tiles, for gfx950 (MI355X): square causal (is_causal=True),
// rectangular (Nq != Nk: cross-attention and chunked prefill) and grouped-query (h query
// heads on h_kv < h K/V heads).  One int8 and one fp16 kernel template; a compile-time
// geometry type (SquareCausal, Rect, Grouped: below) supplies what differs.
//
// Square causal: query row r attends keys j <= r of its own sequence (Nq = Nk = N).  Both kernels keep the
// geometry of the non-causal main kernels, so they consume the unchanged pre-pass outputs (qmha_prepass.hip):
//   one wave = one 32-row query group g, a workgroup of 4 groups shares the LDS-DMA K/V staging
//   (buffer_load ... lds, stages of 2 key tiles, double-buffered), tiles are 32 keys wide.
//   group g visits key tiles t = 0..g; on the diagonal tile t == g a score with j > r is -inf BEFORE the
//   row maximum is formed: no part in the row max, p = 0 exactly, nothing in the row sum, (int8) Pi = 0 and
//   nothing in the P-tile absmax.
//   The workgroup's KV loop ends at the stage that holds its last wave's diagonal tile; later stages are
//   neither staged nor computed.  A wave whose diagonal lies earlier keeps taking part in every barrier
//   and every DMA issue and skips the tile body under a wave-uniform branch (it adds exactly zero).
//   The mask is one select per score under a wave-uniform branch taken on the diagonal tile only, so
//   off-diagonal tiles execute no mask instructions.  (A separate compile-time instantiation of the whole
//   tile body for the diagonal doubled the unrolled loop body and spilled -- fp16 d = 64: 221 VGPRs to
//   scratch at the 4-waves-per-SIMD budget -- so the tile body exists once.)
//   Workgroup cost grows with the q-block index.  fp16: the launch index maps the largest q-blocks of every
//   (b, h) first.  int8: a workgroup runs a PAIR of q-blocks one after the other,
//   nqb - 1 - i and its mirror i: every workgroup of a head then costs the same nqb + 1 units, whatever
//   compute unit it lands on (with heaviest-first single q-blocks, a grid that is resident all at once --
//   B1 H32 N8192 d32 -- ended 1.5x later than its mean: DESIGN.md 10).  The pairs with the largest
//   q-blocks start first; xcd_remap keeps the pairs of one (b, h) in one XCD's L2.
// Rectangular: Q and O are [B, Nq, d_model], K and V [B, Nk, d_model]; Gq = Nq / 32 query groups, Gk = Nk / 32
// key tiles.  The pre-pass touches K and V only and runs unchanged with N = Nk.  Query rows, O rows and `active`
// follow Gq; the K/V bases, the buffer extents, the sK / sV index and the loop bounds follow Gk.
//   diag_off (run-time, wave-uniform, SGPR) is the one switch between the two modes, so each kernel has one
//   rectangular instance per head size:
//     causal, bottom-right aligned (row r attends keys j <= r + Nk - Nq, Nk >= Nq): diag_off = Gk - Gq.  The
//       32-row K/V groups are aligned to the tile grid and Nk - Nq is a multiple of 32, so group g's diagonal
//       tile is exactly key tile g + diag_off and the in-tile mask is the square one (j > r inside the tile);
//       tiles past the diagonal are not visited.
//     non-causal: diag_off = Gk, a diagonal no tile reaches (t <= Gk - 1 < g + Gk): every wave runs all Gk
//       tiles and never takes the mask branch.
//   A wave's last tile is min(g + diag_off, Gk - 1); the workgroup's KV loop ends at the stage holding the last
//   tile of its last active wave, and the partial last stage brings in that many tiles only.  With an offset
//   every int8 workgroup of a head still costs the same; without the mask both passes cost Gk tiles.
// Grouped: Q and O are [B, Nq, h * D], K and V [B, Nk, h_kv * D], G = h / h_kv; the pre-pass runs unchanged with
// H = h_kv, so the workspace holds B * h_kv slices of Nk rows.  The rows, the diagonal and the cached form are Rect's.
//   K/V slice.  The launch index's slice is the K/V slice bh = b * h_kv + kvh (the kernels' H argument is the number
//     of K/V heads, which is h for the other geometries): the K/V bases, the buffer extents and the sK / sV index
//     use it; query rows and O rows keep d_model = h * D and column k * D of query head k.
//   Units.  One K/V slice serves U = G * Gq units: unit u = qg * G + j is query group qg of query head
//     kvh * G + j.  A workgroup holds four consecutive units (nqb = ceil(U / 4)); a wave is active when u < U;
//     diag and last take qg = u / G.  qg is non-decreasing in u, so the workgroup's last tile is that of its last
//     active unit.  With G = 4 a workgroup is the four heads of one query group: one shared diagonal, no wave
//     idle under the mask (decode, Nq = 32: four active waves per workgroup where Rect has one).  G is a
//     run-time, wave-uniform argument (any G >= 2).  For SquareCausal and Rect a unit is a query group of the
//     slice's own head: U = Gq, qg = u, k = kvh.
//   Grid.  B * h_kv * masked_pairs(nqb) for int8 (mirrored unit-block pairs), B * h_kv * nqb for fp16 (heaviest
//     first); xcd_remap keeps the workgroups of one K/V slice on one XCD, so the G heads re-read K/V from its L2.
//   A wave's arithmetic and tile order are those of the Rect instance, so a query head's result is that of the
//   multi-head call on K / V expanded G times, bit for bit.
// Out of range by construction: K/V reads go through buffer descriptors of exactly the (b, kvh) slice
// (Nk * D, Nk * 2D bytes) and a stage issues whole tiles t <= Gk - 1 only; sK / sV are read at t <= Gk - 1
// of slice bh * Gk; Q and O rows are touched by active waves only (u < U: qg < Gq, query head < h).
//
// int8 (fa_tc_int8_b contract): the tile of qmha_fa_int8_kernel -- i8 MFMA for Q@K^T, exact-integer f16
//   MFMA for P@V, one sP per 32x32 tile, the anchored O / l state -- on the Ki / Vh / sK / sV workspace.
// fp16 (fa_tc_v1a contract): the tile of qmha_fa_f16_v3_kernel -- v_mfma_f32_16x16x32_f16 for both
//   products, the lazy base of DESIGN.md 3 -- on the Kh / Vt workspace.
// Both are unpipelined (one tile at a time, co-resident waves interleave); N = 32 is the same kernel
// (one stage, one diagonal tile).
#include "qmha_common.hpp"
#include "qmha_kernels.hpp"

#include <type_traits>

namespace qmha {

static constexpr float kLazySumCapC = 4096.0f;  // the fp16 lazy base's cap
constexpr int kWaves = 4, kSG = 2;

// The geometry of a launch, a kernel argument: the rows of Q / O and of K / V, and which key tiles query
// group g visits -- tiles t <= last(g), masked on tile diag(g).  And the units of a K/V slice (the header's
// "Units"): how many, and which query group and query head unit u is.
// Square causal: the diagonal of group g is tile g, which is also its last; nothing beyond N is passed or
// computed, so these instances carry no offset and no clamp.
struct SquareCausal {
    static constexpr bool kDump = false;
    int N;
    __device__ int nq() const { return N; }
    __device__ int nk() const { return N; }
    __device__ int gk() const { return N / QMHA_GROUP; }
    __device__ int diag(int g) const { return g; }
    __device__ int last(int g) const { return g; }
    __host__ __device__ int units() const { return N / QMHA_GROUP; }
    __device__ int group(int u) const { return u; }
    __device__ int head(int kvh, int u) const { return kvh; }
};
// Rectangular.  causal: bottom-right aligned, diag_off = Gk - Gq (Nk >= Nq, checked by the launchers);
// else diag_off = Gk, a diagonal no tile reaches
struct Rect {
    static constexpr bool kDump = false;
    int Nq, Nk, diag_off;
    Rect(int nq, int nk, bool causal) : Nq(nq), Nk(nk), diag_off(nk / QMHA_GROUP - (causal ? nq / QMHA_GROUP : 0)) {}
    // Host only: the causal geometry of a K/V cache.  The arrays hold `cap` rows per head slice and the
    // first `len` are valid: Nk = cap keeps the bases, the extents and the sK / sV index those of the cache, and the
    // explicit offset (len - nq) / 32 puts the diagonal of the last query group on tile len / 32 - 1, so last(g) <=
    // len / 32 - 1 for every g < Gq and no tile at or beyond len / 32 is staged or computed.  nq <= len <= cap.
    static Rect cached(int nq, int cap, int len) {
        Rect r(nq, cap, false);
        r.diag_off = (len - nq) / QMHA_GROUP;
        return r;
    }
    __device__ int nq() const { return Nq; }
    __device__ int nk() const { return Nk; }
    __device__ int gk() const { return Nk / QMHA_GROUP; }
    __device__ int diag(int g) const { return g + diag_off; }  // >= Gk: none
    __device__ int last(int g) const { return min(g + diag_off, gk() - 1); }
    __host__ __device__ int units() const { return Nq / QMHA_GROUP; }
    __device__ int group(int u) const { return u; }
    __device__ int head(int kvh, int u) const { return kvh; }
};
// Grouped-query: Rect's rows and diagonal (its cached form too), and G query heads per K/V head.  The divisions
// are unsigned: scalar, through a reciprocal, as the launch-index ones are.
struct Grouped : Rect {
    int G;
    Grouped(Rect r, int g) : Rect(r), G(g) {}
    __host__ __device__ int units() const { return G * (Nq / QMHA_GROUP); }
    __device__ int group(int u) const { return (int)((unsigned)u / (unsigned)G); }
    __device__ int head(int kvh, int u) const { return kvh * G + (int)((unsigned)u % (unsigned)G); }
};

// A geometry that also carries the buffers of a dumping instance (int8 kernel; QkDump and PDump in
// qmha_kernels.hpp): the debug hook's twin of a shipped instance, whose own arguments stay as they are.
template <class Geo>
struct Dumping : Geo {
    // the dump's arrays are indexed by the query slice b * h + k, which the kernel takes to be its K/V slice
    static_assert(!std::is_same<Geo, Grouped>::value, "the dump indexes by query slice: Grouped has no twin");
    static constexpr bool kDump = true;
    QkDump qk;
    PDump pd;
    Dumping(Geo g, QkDump q, PDump p) : Geo(g), qk(q), pd(p) {}
};

// Launch index -> (bh, q-block pair): a workgroup runs q-block nqb - 1 - pi and then its mirror pi, so every
// workgroup of a head costs the same nqb + 1 q-block units (the middle q-block of an odd nqb runs alone);
// consecutive indices of an XCD share (b, h), and the pairs holding the largest q-blocks start first.
// (int8 kernel.  The fp16 kernel keeps one q-block per workgroup, heaviest first -- masked_wg_single: with the
// pair loop around it its d = 64 instance no longer fits the 128 VGPRs of four waves per SIMD, 4 spilled, and
// it has no grid that is resident all at once among the measured shapes.)
__host__ __device__ constexpr int masked_pairs(int nqb) { return (nqb + 1) / 2; }
__device__ __forceinline__ void masked_wg_single(int nqb, int& bh, int& qb) {
    const int wg = xcd_remap(blockIdx.x, gridDim.x);
    bh = wg / nqb;
    qb = nqb - 1 - wg % nqb;
}
__device__ __forceinline__ void masked_wg(int nqb, int& bh, int& pi) {
    const int wg = xcd_remap(blockIdx.x, gridDim.x);
    bh = wg / masked_pairs(nqb);
    pi = wg % masked_pairs(nqb);
}

// K/V staging of both kernels: fixed per-lane source offsets (the LDS image's swizzle applied to the
// source address by the kernel that fills koff / voff), the stage offset in soffset.
template <int WAVES, int KCH, int VCH, int KBYTES, int VBYTES, int SG>
struct MaskedStager {
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

// ---------------------------------------------------------------------------------------
// int8: 32x32 accumulator map.  Lane (col, half) holds S^T[acc_row(r, half)][col], r = 0..15: query
// row `col` of the group against key acc_row(r, half) of the tile, so on the diagonal tile (the groups of
// queries and keys aligned) the score of register r is masked when acc_row(r, half) > col.
// ---------------------------------------------------------------------------------------
template <int D, class Geo>
__global__ __launch_bounds__(kWaves * 64, D > 64 ? 2 : 4) void qmha_fa_int8_masked_kernel(
    const float* __restrict__ Qf, const int8_t* __restrict__ Ki, const _Float16* __restrict__ Vh,
    const float* __restrict__ sK, const float* __restrict__ sV, float* __restrict__ O, Geo geo, int H, int d_model,
    int nqb, float c_log2) {
    constexpr int WAVES = kWaves, SG = kSG;
    constexpr int KS = D / 32;               // i8 MFMA k-steps (QK) and d-blocks (PV)
    constexpr int KBYTES = SG * 32 * D;      // K int8 per stage
    constexpr int VBYTES = SG * 32 * D * 2;  // V f16 per stage
    constexpr int KCH = KBYTES / 16, VCH = VBYTES / 16;
    constexpr bool DUMP = Geo::kDump;  // also store what the kernel computed (Dumping<Geo>), per tile a wave runs
    static_assert(D == 32 || D == 64 || D == 128, "masked int8: d in {32, 64, 128}");
    static_assert(KCH % 64 == 0 && VCH % 64 == 0 && (KCH / SG) % 64 == 0, "whole KiB LDS-DMA pieces");
    __shared__ __attribute__((aligned(16))) char lds[2][KBYTES + VBYTES];

    const int Nq = geo.nq(), Nk = geo.nk();
    const int Gq = Nq / QMHA_GROUP, Gk = geo.gk(), U = geo.units();
    int bh, pi;
    masked_wg(nqb, bh, pi);
    const int b = bh / H, kvh = bh % H;  // bh: the K/V slice (H K/V heads)
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int half = lane >> 5, col = lane & 31;
#pragma nounroll
    for (int pass = 0; pass < 2; ++pass) {  // the pair's large q-block, then its mirror (uniform)
    const int qb = pass == 0 ? nqb - 1 - pi : pi;
    if (pass == 1 && pi == nqb - 1 - pi) break;  // odd nqb: the middle q-block has no partner
    const int u = qb * WAVES + wave;
    const bool active = u < U;  // wave-uniform; an inactive wave still stages and syncs
    const int qg = geo.group(u), k = geo.head(kvh, u);  // query group, query head
    // the workgroup's last tile: that of its last active wave
    const int wg_last = geo.last(geo.group(min(qb * WAVES + WAVES - 1, U - 1)));
    const int nst = wg_last / SG + 1;
    const int my_diag = geo.diag(qg);              // this wave's diagonal tile
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
        if constexpr (DUMP) {  // the Q operand as held in registers: lane (col, half), k-step s
            int8_t* qd = geo.qk.Qi + ((size_t)bh * Nq + (size_t)qg * QMHA_GROUP + col) * D + 16 * half;
#pragma unroll
            for (int s = 0; s < KS; ++s) *reinterpret_cast<v4i*>(qd + 32 * s) = qop[s];
            if (lane == 0) geo.qk.sQ[(size_t)bh * Gq + qg] = sq;
        }
    } else {
#pragma unroll
        for (int s = 0; s < KS; ++s) qop[s] = v4i{0, 0, 0, 0};
    }
    size_t drow = 0;  // DUMP: this lane's query row
    if constexpr (DUMP) drow = (size_t)bh * Nq + (size_t)qg * QMHA_GROUP + col;
    v16f o[KS];
#pragma unroll
    for (int m = 0; m < KS; ++m) o[m] = v16f{};
    float m_run = 0.0f;   // m0 = 0 (fa_tc_int8_b.cu:402), log2 units
    float l_run = 0.0f;   // anchored: l * 2^(m - anchor), over this lane's half of the keys
    float anchor = 0.0f;  // o = O * 2^(m - anchor), anchor <= m

    const char* kbase = reinterpret_cast<const char*>(Ki + (size_t)bh * Nk * D);
    const char* vbase = reinterpret_cast<const char*>(Vh + (size_t)bh * Nk * D);
    const float* skb = sK + (size_t)bh * Gk;
    const float* svb = sV + (size_t)bh * Gk;

    MaskedStager<WAVES, KCH, VCH, KBYTES, VBYTES, SG> stg;
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
        if constexpr (DUMP) {  // S^T of tile t before the mask (32x32 accumulator map); only an active wave gets here
            int32_t* sd = geo.qk.S + drow * Nk + (size_t)t * QMHA_GROUP;
#pragma unroll
            for (int r = 0; r < 16; ++r) sd[acc_row(r, half)] = s[r];
        }
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
        // Pi = rint(p/sP) (0..127), carried as the f16 subnormal Pi * 2^-24 as in qmha_fa_int8_pipe_kernel:
        // fma(p, 1/sP, 1.5 * 2^23) rounds half-even to an integer whose float bits end in Pi, and those low
        // 16 bits are the f16 encoding of Pi * 2^-24; one byte permute packs two entries.  P@V then yields
        // T * 2^-24 exactly (T < 2^20) and the O scale carries the 2^24 back.
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
        if constexpr (DUMP) {
            if (half == 0) geo.pd.m[drow * Gk + t] = m_new;
            if (lane == 0) geo.pd.sP[((size_t)bh * Gq + qg) * Gk + t] = sp;
            dump_p_operand<true>(geo.pd.Pi + drow * Nk + (size_t)t * QMHA_GROUP, pop, half);
        }
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
            if constexpr (DUMP)
                dump_pv_acc<true>(geo.pd.T + (((size_t)bh * Gk + t) * Nq + qg * QMHA_GROUP + col) * D + 32 * m, acc, half);
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
        if constexpr (DUMP) {
            if (half == 0) geo.pd.l[drow] = l;
        }
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
// fp16: 16x16 accumulator map (qmha_fa_f16_v3_kernel).  Lane l = 16 grp + r16 holds, per query block
// qb, S^T[kap16(kb, 4 grp + i)][16 qb + r16] (kb = 0, 1, i = 0..3): on the diagonal tile that score
// is masked when kap16(kb, 4 grp + i) > 16 qb + r16.
// ---------------------------------------------------------------------------------------
template <int D, class Geo>
__global__ __launch_bounds__(kWaves * 64, D > 64 ? 2 : 4) void qmha_fa_f16_masked_kernel(
    const float* __restrict__ Qf, const _Float16* __restrict__ Kh, const _Float16* __restrict__ Vt,
    float* __restrict__ O, Geo geo, int H, int d_model, int nqb, float c_log2) {
    QMHA_ENABLE_AGPR_MFMA();
    asm volatile("" : "+v"(c_log2));  // a VOP3 fma reading an SGPR issues at the slow rate
    constexpr int WAVES = kWaves, SG = kSG;
    constexpr int KS = D / 32;            // QK k-steps (K = 32)
    constexpr int DB = D / 16;            // PV d-blocks of 16 rows
    constexpr int RB = 2 * D;             // K row bytes
    constexpr int KBYTES = SG * 32 * RB;  // K per stage
    constexpr int VBYTES = SG * 32 * D * 2;
    constexpr int KCH = KBYTES / 16, VCH = VBYTES / 16;
    static_assert(D == 64 || D == 128, "masked fp16: d in {64, 128}");
    static_assert(KCH % 64 == 0 && VCH % 64 == 0 && (KCH / SG) % 64 == 0, "whole KiB LDS-DMA pieces");
    __shared__ __attribute__((aligned(16))) char lds[2][KBYTES + VBYTES];

    const int Nq = geo.nq(), Nk = geo.nk();
    const int U = geo.units();
    int bh, qb0;
    masked_wg_single(nqb, bh, qb0);
    const int b = bh / H, kvh = bh % H;  // bh: the K/V slice (H K/V heads)
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int u = qb0 * WAVES + wave;
    const bool active = u < U;
    const int qg = geo.group(u), k = geo.head(kvh, u);  // query group, query head
    const int grp = lane >> 4, r16 = lane & 15;
    const int wg_last = geo.last(geo.group(min(qb0 * WAVES + WAVES - 1, U - 1)));  // of the last active wave
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

    const char* kbase = reinterpret_cast<const char*>(Kh + (size_t)bh * Nk * D);
    const char* vbase = reinterpret_cast<const char*>(Vt + (size_t)bh * Nk * D);

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
        const uint64_t over0 = __builtin_amdgcn_ballot_w64(ts[0] > kLazySumCapC);
        const uint64_t over1 = __builtin_amdgcn_ballot_w64(ts[1] > kLazySumCapC);
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
// host launchers: square causal calls take the SquareCausal instances, grouped calls (Hkv < H) the Grouped ones,
// everything else the Rect ones
// ---------------------------------------------------------------------------------------
static bool masked_shape_ok(int Nq, int Nk, bool causal) {
    return Nq >= QMHA_GROUP && Nk >= QMHA_GROUP && Nq % QMHA_GROUP == 0 && Nk % QMHA_GROUP == 0 && !(causal && Nk < Nq);
}
// K/V cache: a cache of `cap` rows of which `len` are valid, Nk = cap.  causal: Rect::cached; else
// every row attends all cap rows, so len == cap.
static bool cached_shape_ok(int Nq, int cap, int len, bool causal) {
    if (!masked_shape_ok(Nq, cap, false) || len % QMHA_GROUP != 0) return false;
    return causal ? Nq <= len && len <= cap : len == cap;
}
static Rect cached_geo(int Nq, int cap, int len, bool causal) { return causal ? Rect::cached(Nq, cap, len) : Rect(Nq, cap, false); }
static bool grouped_heads_ok(int B, int H, int Hkv, int D, int d_model) {
    return B >= 1 && Hkv >= 1 && Hkv < H && H % Hkv == 0 && d_model == H * D;
}
static int masked_nqb(int units) { return (units + kWaves - 1) / kWaves; }  // unit blocks per K/V slice

// The geometry of a call of its own, checked, handed to `launch`
template <class Launch>
static hipError_t masked_call(int Nq, int Nk, bool causal, Launch&& launch) {
    if (!masked_shape_ok(Nq, Nk, causal)) return hipErrorInvalidValue;
    return causal && Nq == Nk ? launch(SquareCausal{Nq}) : launch(Rect(Nq, Nk, causal));
}

// Launch the instance of `geo`, which the caller has checked, over B * H K/V slices
template <class Geo>
static hipError_t fa_int8_masked_launch(const Int8Workspace& w, const float* Qf, float* O, int B, int H, int D, int d_model,
                                        hipStream_t stream, Geo geo) {
    const int nqb = masked_nqb(geo.units());
    auto launch = [&](auto d) {
        hipLaunchKernelGGL((qmha_fa_int8_masked_kernel<decltype(d)::value, Geo>), dim3(B * H * masked_pairs(nqb)), dim3(kWaves * 64), 0,
                           stream, Qf, w.Ki, w.Vh, w.sK, w.sV, O, geo, H, d_model, nqb, softmax_scale_log2(D));
        return hipGetLastError();
    };
    switch (D) {
        case 32: return launch(std::integral_constant<int, 32>{});
        case 64: return launch(std::integral_constant<int, 64>{});
        case 128: return launch(std::integral_constant<int, 128>{});
        default: return hipErrorInvalidValue;
    }
}

hipError_t launch_fa_int8_masked_main(const Int8Workspace& w, const float* Qf, float* O, int B, int Nq, int Nk, int H, int D,
                                      int d_model, bool causal, hipStream_t stream) {
    return masked_call(Nq, Nk, causal, [&](auto geo) { return fa_int8_masked_launch(w, Qf, O, B, H, D, d_model, stream, geo); });
}

// The dumping twin of the instance launch_fa_int8_masked_main launches for this shape: the same grid and
// arguments, the geometry wrapped in Dumping<>
hipError_t launch_fa_int8_masked_pstage_dump(const Int8Workspace& w, const float* Qf, float* O, int B, int Nq, int Nk, int H,
                                             int D, int d_model, bool causal, QkDump dbg, PDump pd) {
    return masked_call(Nq, Nk, causal, [&](auto geo) {
        return fa_int8_masked_launch(w, Qf, O, B, H, D, d_model, nullptr, Dumping<decltype(geo)>(geo, dbg, pd));
    });
}

template <class Geo>
static hipError_t fa_f16_masked_launch(const F16Workspace& w, const float* Qf, float* O, int B, int H, int D, int d_model,
                                       hipStream_t stream, Geo geo) {
    const int nqb = masked_nqb(geo.units());
    auto launch = [&](auto d) {
        hipLaunchKernelGGL((qmha_fa_f16_masked_kernel<decltype(d)::value, Geo>), dim3(B * H * nqb), dim3(kWaves * 64), 0, stream, Qf,
                           w.Kh, w.Vt, O, geo, H, d_model, nqb, softmax_scale_log2(D));
        return hipGetLastError();
    };
    switch (D) {
        case 64: return launch(std::integral_constant<int, 64>{});
        case 128: return launch(std::integral_constant<int, 128>{});
        default: return hipErrorInvalidValue;
    }
}

hipError_t launch_fa_f16_masked_main(const F16Workspace& w, const float* Qf, float* O, int B, int Nq, int Nk, int H, int D,
                                     int d_model, bool causal, hipStream_t stream) {
    return masked_call(Nq, Nk, causal, [&](auto geo) { return fa_f16_masked_launch(w, Qf, O, B, H, D, d_model, stream, geo); });
}

// K/V cache: always the Rect instances (also at Nq == len, where a call of its own takes the SquareCausal ones)
hipError_t launch_fa_int8_masked_cached(const Int8Workspace& w, const float* Qf, float* O, int B, int Nq, int cap, int len,
                                        int H, int D, int d_model, bool causal, hipStream_t stream) {
    if (!cached_shape_ok(Nq, cap, len, causal)) return hipErrorInvalidValue;
    return fa_int8_masked_launch(w, Qf, O, B, H, D, d_model, stream, cached_geo(Nq, cap, len, causal));
}

hipError_t launch_fa_f16_masked_cached(const F16Workspace& w, const float* Qf, float* O, int B, int Nq, int cap, int len,
                                       int H, int D, int d_model, bool causal, hipStream_t stream) {
    if (!cached_shape_ok(Nq, cap, len, causal)) return hipErrorInvalidValue;
    return fa_f16_masked_launch(w, Qf, O, B, H, D, d_model, stream, cached_geo(Nq, cap, len, causal));
}

// Grouped-query (Hkv < H): always the Grouped instances, for every Nq and Nk, over B * Hkv K/V slices
hipError_t launch_fa_int8_gqa_main(const Int8Workspace& w, const float* Qf, float* O, int B, int Nq, int Nk, int H, int Hkv,
                                   int D, int d_model, bool causal, hipStream_t stream) {
    if (!grouped_heads_ok(B, H, Hkv, D, d_model) || !masked_shape_ok(Nq, Nk, causal)) return hipErrorInvalidValue;
    return fa_int8_masked_launch(w, Qf, O, B, Hkv, D, d_model, stream, Grouped(Rect(Nq, Nk, causal), H / Hkv));
}

hipError_t launch_fa_f16_gqa_main(const F16Workspace& w, const float* Qf, float* O, int B, int Nq, int Nk, int H, int Hkv,
                                  int D, int d_model, bool causal, hipStream_t stream) {
    if (!grouped_heads_ok(B, H, Hkv, D, d_model) || !masked_shape_ok(Nq, Nk, causal)) return hipErrorInvalidValue;
    return fa_f16_masked_launch(w, Qf, O, B, Hkv, D, d_model, stream, Grouped(Rect(Nq, Nk, causal), H / Hkv));
}

hipError_t launch_fa_int8_gqa_cached(const Int8Workspace& w, const float* Qf, float* O, int B, int Nq, int cap, int len, int H,
                                     int Hkv, int D, int d_model, bool causal, hipStream_t stream) {
    if (!grouped_heads_ok(B, H, Hkv, D, d_model) || !cached_shape_ok(Nq, cap, len, causal)) return hipErrorInvalidValue;
    return fa_int8_masked_launch(w, Qf, O, B, Hkv, D, d_model, stream, Grouped(cached_geo(Nq, cap, len, causal), H / Hkv));
}

hipError_t launch_fa_f16_gqa_cached(const F16Workspace& w, const float* Qf, float* O, int B, int Nq, int cap, int len, int H,
                                    int Hkv, int D, int d_model, bool causal, hipStream_t stream) {
    if (!grouped_heads_ok(B, H, Hkv, D, d_model) || !cached_shape_ok(Nq, cap, len, causal)) return hipErrorInvalidValue;
    return fa_f16_masked_launch(w, Qf, O, B, Hkv, D, d_model, stream, Grouped(cached_geo(Nq, cap, len, causal), H / Hkv));
}

}  // namespace qmha

