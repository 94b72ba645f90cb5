// qmha_fp8_band.hip -- the windowed prefill call of an e4m3 K/V cache, with attention sinks (fa_tc_fp8) for
// gfx950 (MI355X), in a translation unit of its own so that every other kernel keeps its bytes.  qmha_fa_fp8.hip's attend
// takes any number of query rows but sweeps every sequence from key 0 and has no sink; qmha_fp8_decode_window.hip's call
// has the window and the sinks but packs at most 32 query rows into MFMA columns.  A local layer's prefill chunk (Mistral,
// Gemma 2/3: windows of 1024 or 4096; gpt-oss: 128 plus a learned sink per head) needs both: any Nq, and per row the last
// `window` keys only.
//
// The contract (include/launchers.h): with e_r = lens[b] - Nq + r, row r sees key j iff e_r - window < j <= e_r; head k's
// softmax has one more column sinks[k] (natural-log units of S / sqrt(d)) with no value row; the arithmetic per row is the
// fp8 attend's, tiles ascending from the zero state.
//
// Work split: the fp8 attend's.  One wave is a 32-row query group of the padded block of Ragged::of (absolute row
// positions keep their 32-row groups), kWaves of them are the units of one unit block under Grouped's unit map and share
// the LDS-DMA stages of two key tiles, double-buffered; S^T = K Q^T and O^T = V^T P^T run on
// v_mfma_f32_16x16x32_fp8_fp8 with that kernel's operand reads (one ds_read_b128 of a row-major K row feeds two MFMAs, the
// V^T block of fp8_vt_offset), its ballot-guarded TRUE running maximum and its epilogue.  What is its own:
//   band       query group qg has diagonal tile dg = diag(qg), whose row 16 qb + r16 ends at key 32 dg + 16 qb + r16.  Its
//              sweep is tiles first(qg) = max(0, 32 dg - window + 1) / 32 ... last(qg) = dg: the tile of the first key its
//              first row sees up to the diagonal.
//   stages     a workgroup's first stage starts at t0 = first(group of its first unit) & ~1 -- first() is monotone in the
//              unit --, and nst counts stages from t0: tiles before t0 are neither staged nor computed.  Stage st of the
//              workgroup is stage t0 / 2 + st of the sequence, issued as the fp8 attend issues that stage.
//   waves      each wave carries my_first and my_last and skips, wave-uniformly, the tiles outside that range in the stages
//              it helps to issue.  With G % 4 == 0 the four waves are four heads of one query group: one band, every stage
//              shared.  At G < 4 the waves' bands are staggered and a stage serves the waves whose bands reach it.
//   left edge  a select to -inf before the maximum on the tiles with 32 t <= 32 dg + 31 - window (wave-uniform; at most two
//              per sweep): key 32 t + key0 + i + 8 kb is hidden iff it is <= 32 dg + 16 qb + r16 - window.  Independent of
//              the diagonal's select: for window < 32 both fire on the diagonal tile.  A row with no visible key in a tile
//              keeps its state: its scores are -inf, its maximum does not move (alpha is exactly 1) and its p are 0.
//   sink       O = v_scale * o / (l + 2^(min(sink_k log2(e) - m + 8, 120))): m the row's true running maximum after its last
//              tile, the term added to the lane-joined l last; sinks[k] is read for real heads by active waves only.
//   paged      the verdict of a sequence reads the table columns whose pages hold rows [32 t0_min, L) only (t0_min: unit
//              block 0's t0, the same in every workgroup of the sequence), and the walk begins at the workgroup's t0.
// With window >= lens[b] and no sinks every sweep starts at tile 0, no real row's score is changed by the left select and
// the statements are the fp8 attend's: O is attend_tokens' / attend_paged's, bit for bit.
// No scratch, no atomics, no waiting on another workgroup: one plain launch.
#include "qmha_fa_masked.hpp"
#include "qmha_fp8.hpp"

#include <utility>

namespace qmha {

// the window and the sinks of a call
struct Band {
    int window;          // keys a row sees, >= 1
    const float* sinks;  // DEVICE float32 [h], or null
    // the first tile of the sweep of a query group whose diagonal tile is dg (32 dg <= 2^30, window <= INT_MAX: no overflow)
    __device__ int first(int dg) const { return max(0, QMHA_GROUP * dg - window + 1) / QMHA_GROUP; }
};

// (d = 64 keeps the fp8 attend's bound of four waves per SIMD: the band's words take it from that kernel's 93 VGPRs to 99, one
// occupancy step below its five; asked for five it fits 96 only with 12 bytes of scratch memory, which this call does not use.)
template <class Geo, int D>
__global__ __launch_bounds__(kWaves * 64, D > 64 ? 2 : 4) void qmha_fp8_band_kernel(
    const float* __restrict__ Qf, const uint8_t* __restrict__ K8, const uint8_t* __restrict__ Vt8, float* __restrict__ O, Geo any, Band band,
    const int32_t* __restrict__ lens, int H, int d_model, int nqb, float q_scale, float s_log2, float v_scale) {
    static_assert(kRaggedGeo<Geo> && !kSplitGeo<Geo> && !kPackedGeo<Geo> && !kWindowGeo<Geo>, "Ragged or Paged");
    // the sequence's verdict: workgroup-uniform, before the first barrier or DMA issue.  A length outside [Nq, cap], or
    // (Paged) a table entry outside the pool among the columns of rows [32 t0_min, L): the sequence's Nq rows of O are
    // zeros -- written by the first workgroup of each K/V slice, its G heads' columns -- and none of its K/V is read
    int bh, qb0;
    masked_wg_single(nqb, bh, qb0);
    const int L = __builtin_amdgcn_readfirstlane(lens[bh / H]);
    bool valid = any.valid(L);
    const Geo geo = any.of(valid ? L : any.Nq);
    if constexpr (kPagedGeo<Geo>) {
        if (valid) valid = any.used_pages_ok(bh / H, QMHA_GROUP * (band.first(geo.diag(0)) & ~(kSG - 1)), L);
    }
    if (!valid) {
        if (qb0 == 0) zero_real_rows<D>(O, any, bh, H, d_model);
        return;
    }

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
    if (qb0 * WAVES >= U) return;  // the grid follows the host's Nq, U the sequence's length: no active unit, no barrier
    const int u = qb0 * WAVES + wave;
    const bool active = u < U;
    const int qg = geo.group(u), k = geo.head(kvh, u);  // query group, query head
    const int grp = lane >> 4, r16 = lane & 15;
    const int wg_last = geo.last(geo.group(min(qb0 * WAVES + WAVES - 1, U - 1)));  // of the last active wave
    const int t0 = band.first(geo.diag(geo.group(qb0 * WAVES))) & ~(SG - 1);        // of the first: the first stage's first tile
    const int nst = (wg_last - t0) / SG + 1;                                          // stages from t0; wg_last >= t0
    const int my_diag = geo.diag(qg);
    const int my_first = band.first(my_diag);
    const int my_last = active ? geo.last(qg) : -1;
    // tiles t <= my_left hold a key the group's last row does not see: they take the left select
    const int my_left = (QMHA_GROUP * my_diag + QMHA_GROUP - 1 - band.window) >> 5;  // floor: negative where there is none

    // Q into the QK B operand: query 16 qb + r16, bytes d = 64 kp + 16 grp + 8 h .. +7 for k-step 2 kp + h
    fp8x8 qop[2][2 * KP];
#pragma unroll
    for (int qb = 0; qb < 2; ++qb)
#pragma unroll
        for (int ks = 0; ks < 2 * KP; ++ks) {
            float x[8] = {};
            if (active && row_real(geo, qg * QMHA_GROUP + 16 * qb + r16)) {  // a pad lane loads nothing
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
    // stage st of the workgroup is stage t0 / 2 + st of the sequence (t0 is even).  Paged: the stage's page slice is the
    // buffer, the stage offset the stage's place in its page; the walk starts at t0, whose column and every later one up
    // to L's passed used_pages_ok (t0 >= t0_min).  Only tiles <= wg_last come in.
    std::conditional_t<kPagedGeo<Geo>, PageWalk, NoWalk> walk;
    if constexpr (kPagedGeo<Geo>) walk.start_at(geo, b, t0);
    auto issue = [&](int buf, int st) {
        const int ts = t0 + st * SG, ngr = min(SG, wg_last + 1 - ts);
        if constexpr (kPagedGeo<Geo>) {
            walk.take(geo);
            const size_t slice = (size_t)walk.page * H + kvh, pbytes = (size_t)geo.PG * (QMHA_GROUP * D);
            stg.issue(lds[buf], reinterpret_cast<const char*>(K8) + slice * pbytes, (int)pbytes,
                      reinterpret_cast<const char*>(Vt8) + slice * pbytes, (int)pbytes, walk.sip, ngr, wave);
            walk.advance(geo, b);
        } else
            stg.issue(lds[buf], kbase, Nk * RB, vbase, Nk * D, ts / SG, ngr, wave);
    };
    // S^T blocks [kb][qb] of tile gi: rows kap16(kb, .) of the K tile against query block qb
    struct S4 {
        v4f v[2][2];
    };
    auto qk = [&](const char* Lb, int gi) {
        S4 s;
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
            const int krow = gi * 32 + kap16(kb, r16);
            s.v[kb][0] = s.v[kb][1] = v4f{};
#pragma unroll
            for (int kp = 0; kp < KP; ++kp) {
                const v2l kop = *reinterpret_cast<const v2l*>(Lb + krow * RB + 16 * ((4 * kp + grp) ^ kswz16<RB>(krow)));
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
    auto tile = [&](const char* Lb, int gi, S4 s, int t, bool diag, bool left) {
        v2l vop[DB / 2];  // V^T rows 32 mp + r16 and + 16, slots 8 grp .. +7 (read before the softmax)
#pragma unroll
        for (int mp = 0; mp < DB / 2; ++mp) {
            const int line = 16 * mp + r16;
            vop[mp] = *reinterpret_cast<const v2l*>(Lb + KBYTES + gi * 32 * D + line * 64 + 16 * (grp ^ vswz16(line)));
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
        if (left) {  // wave-uniform: the tile holds a key some row of the group sees no more
            // key c of the tile is hidden from row 16 qb + r16 iff c <= hid + 16 qb; the scalar part is >= -31 on such a tile
            const int hid = (QMHA_GROUP * (my_diag - t) - band.window) + (int)(threadIdx.x & 15);
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int qb = 0; qb < 2; ++qb)
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        s.v[kb][qb][i] = key0 + i + 8 * kb <= hid + 16 * qb ? -__builtin_huge_valf() : s.v[kb][qb][i];
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
        const int ts = t0 + st * SG;
        if (ts <= my_last && ts + SG > my_first) {  // wave-uniform: the stage holds a tile of this wave's band
            const char* Lb = lds[buf];
#pragma unroll
            for (int gi = 0; gi < SG; ++gi) {
                const int t = ts + gi;
                if (t >= my_first && t <= my_last) tile(Lb, gi, qk(Lb, gi), t, t == my_diag, t <= my_left);
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
        const float sink = band.sinks ? band.sinks[k] * kLog2e : 0.0f;  // k: a real head
#pragma unroll
        for (int qb = 0; qb < 2; ++qb) {
            float l = l_run[qb];
            l += __shfl_xor(l, 16);
            l += __shfl_xor(l, 32);
            // the sink's column: 2^(sink log2(e) - m + 8), mb = m - 8; the exponent clamped, so finite for every finite sink
            if (band.sinks) l += __builtin_amdgcn_exp2f(fminf(sink - mb[qb], 120.0f));
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
// host: masked_geo's Ragged / Paged geometry of a token-granular call; the fp8 attend's grid
// ---------------------------------------------------------------------------------------
template <class Geo>
static hipError_t fp8_band_launch(const Fp8Workspace& w, const float* Qf, float* O, const MaskedCall& c, const Band& band, hipStream_t stream,
                                  Geo geo) {
    const int nqb = masked_nqb(grid_units(geo));
    const dim3 grid(c.B * c.Hkv * nqb), block(kWaves * 64);
    return fp8_cache_d(c.D, [&](auto d) {
        hipLaunchKernelGGL((qmha_fp8_band_kernel<Geo, decltype(d)::value>), grid, block, 0, stream, Qf, w.K8, w.Vt8, O, geo, band, c.lens, c.Hkv,
                           c.d_model, nqb, w.q_scale, w.q_scale * w.k_scale * softmax_scale_log2(c.D), w.v_scale);
        return hipGetLastError();
    });
}

hipError_t launch_fp8_band(const Fp8Workspace& w, const float* Qf, float* O, const MaskedCall& c, int window, const float* sinks,
                           hipStream_t stream) {
    if (!c.ragged || window < 1) return hipErrorInvalidValue;
    return masked_geo(c, [&](auto geo) {
        if constexpr (kRaggedGeo<decltype(geo)>) return fp8_band_launch(w, Qf, O, c, Band{window, sinks}, stream, geo);
        else return hipErrorInvalidValue;
    });
}

}  // namespace qmha
