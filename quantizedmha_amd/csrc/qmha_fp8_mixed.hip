// qmha_fp8_mixed.hip -- the mixed-step calls of an e4m3 K/V cache (fa_tc_fp8) for gfx950 (MI355X), in a
// translation unit of its own so that every other kernel keeps its bytes.  A continuous-batching step holds a few sequences
// in chunked prefill beside many that decode one row.  The shipped fp8 attends take one host Nq for the whole batch, so
// such a step costs a launch group per distinct row count; the int8 / fp16 packed call sizes its grid by B x max_nq and
// sweeps a decoding sequence with one wave per query head.  Here Q, O, K and V have no batch axis: sequence
// b owns the rows [cu[b], cu[b + 1]) (cu: DEVICE int32 [B + 1], read when the kernels run), nq_b = cu[b + 1] - cu[b], and
// the grid is sized from `total` and B alone.
//
// The kind of a sequence is decided on the device: G nq_b <= 32 is the decode kind, whose rows of O are
// qmha_fp8_decode_window.hip's bits at Nq = nq_b (its one-launch form where that call has one chunk); any other the prefill
// kind, whose rows are qmha_fp8_band.hip's.  The statements of both bodies are restated here, not shared through a header.
//
// qmha_fp8_mixed_kernel: one launch over a flattened item space, a workgroup of four waves per item.
//   prefill items  [0, Hkv PB): item (kvh, i), PB = mixed_prefill_blocks(total, B, G) >= the unit blocks of all sequences
//                  (a sequence has Ga_b <= nq_b / 32 + 2 query groups under Ragged::of and ceil(Ga_b G / 4) unit blocks).
//                  Every wave finds (b, block) of i from the same words: lanes take sequences b = lane + 64 j, form
//                  count_b -- 0 for an empty, out-of-range or decode-kind sequence, 1 for a prefill-kind one with a length
//                  outside [nq_b, cap] (its rows are zeroed), ceil(Ga_b G / 4) otherwise --, and a wave prefix sum with a
//                  running base locates i.  An item beyond the sum leaves before any barrier.  The long work comes first.
//   decode items   Hkv PB + ((b Hkv + kvh) NCw + c), NCw = mixed_chunks(cap, G, window, chunk_rows): the chunks of the
//                  windowed decode call at its widest query block, 32 / G rows.  An item of a prefill-kind, empty or
//                  out-of-range sequence leaves at once; so does chunk c >= nc_b = decode_window_chunks(cap, nq_b, ..),
//                  the chunks the shipped call would launch.  nc_b == 1: the item adds the sink and writes O itself.
// qmha_fp8_mixed_combine_kernel: launched when NCw > 1, for the decode-kind sequences with nc_b > 1, over a scratch
//   indexed (b NCw + c) (32 / G) + r.
// qmha_fp8_mixed_rows_kernel: the append, a wave per (tensor, K/V head, touched 32-row group), located by the same scan
//   over count_b = groups touched by [pos[b], pos[b] + n_b); the K row and V^T dword rules of qmha_kv_fp8.hip.
//
// Every index formed from cu: r0 = cu[b], r1 = cu[b + 1] are used only after 0 <= r0 <= r1 <= total, and then only as
// rows r0 + r, r < r1 - r0.  counts are clamped to the grid's bound before they are summed (no overflow; the host refuses
// a bound above INT_MAX / 65).  With a cu whose ranges overlap the sum can exceed the bound: items past it do not exist,
// rows stay unwritten, nothing leaves the buffers.
// No atomics, no flags, no waiting on another workgroup; every store is a vector store.
#include "qmha_fa_masked.hpp"
#include "qmha_fp8.hpp"

#include <limits.h>
#include <utility>

namespace qmha {
namespace mixed {

// the operands of a call that are not the cache's
struct Step {
    const int32_t* cu;   // DEVICE int32 [B + 1]
    int total, B;        // rows of Q and O, sequences
    int window;          // keys a row sees, >= 1
    const float* sinks;  // DEVICE float32 [h], or null
    float *Oc, *pm, *pl;  // the decode kind's partials: [B][NC][RQ][h D], [B][NC][RQ][h], [B][NC][RQ][h]
    int C, NC, RQ;       // tiles per chunk (even), chunks NCw, rows of a slice 32 / G
    int PB;              // prefill items per K/V head
};

// sequence b's rows: false for a range that must not become an address, or an empty one
__device__ __forceinline__ bool seq_rows(const Step& s, int b, int& r0, int& nq) {
    r0 = s.cu[b];
    const int r1 = s.cu[b + 1];
    nq = r1 - r0;
    return r0 >= 0 && r1 > r0 && r1 <= s.total;
}

// Item idx of the flattened space of count(b) items per sequence: lanes take b = lane + 64 j, an inclusive wave prefix sum
// with a running base finds the sequence and the item's place in it.  Wave-uniform results; false: idx is beyond the sum.
// count(b) <= limit, 65 limit <= INT_MAX.
template <class Count>
__device__ __forceinline__ bool locate(int B, int idx, Count&& count, int& b_out, int& blk_out) {
    const int lane = threadIdx.x & 63;
    int base = 0;
    for (int b0 = 0; b0 < B; b0 += 64) {
        const int n = b0 + lane < B ? count(b0 + lane) : 0;
        int incl = n;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int t = __shfl_up(incl, d);
            if (lane >= d) incl += t;
        }
        const unsigned long long hit = __builtin_amdgcn_ballot_w64(base + incl > idx);
        if (hit) {
            const int src = __builtin_ctzll(hit);
            b_out = b0 + src;
            blk_out = idx - base - __builtin_amdgcn_readlane(incl - n, src);
            return true;
        }
        base += __builtin_amdgcn_readlane(incl, 63);  // <= idx
    }
    return false;
}

// rows [r0, r0 + nq) of O, the G heads' columns of K/V head kvh: in bounds by the range test
template <int D>
__device__ __forceinline__ void zero_rows(float* __restrict__ O, int r0, int nq, int G, int kvh, int d_model) {
    const int W4 = G * D / 4;  // 16-byte pieces of a row's G heads
    float* o = O + (size_t)r0 * d_model + (size_t)kvh * G * D;
    for (int i = threadIdx.x; i < nq * W4; i += kWaves * 64) *reinterpret_cast<v4f*>(o + (size_t)(i / W4) * d_model + 4 * (i % W4)) = v4f{};
}

__device__ __forceinline__ int band_first(int window, int dg) { return max(0, QMHA_GROUP * dg - window + 1) / QMHA_GROUP; }
// 2^(sink log2(e) - m + 8) for a maximum given less its bias of 8, the exponent clamped: finite for every finite sink
__device__ __forceinline__ float sink_term(float sink, float m_less_bias) {
    return __builtin_amdgcn_exp2f(fminf(sink * kLog2e - m_less_bias, 120.0f));
}
__device__ __forceinline__ int window_t0(int L, int Nq, int window) { return max(0, L - Nq - window + 1) / (kSG * QMHA_GROUP) * kSG; }
// decode_window_chunks (qmha_kernels.hpp) on the device
__device__ __forceinline__ int window_chunks(int cap, int Nq, int window, int C) {
    const long long span = (long long)Nq + window + 62, rows = span < cap ? span : cap;
    return ((int)((rows + 31) / 32) + C - 1) / C;
}

template <int D>
struct Tiles {
    static constexpr int WAVES = kWaves, SG = kSG;
    static constexpr int KP = D / 64;            // 16-byte chunks a lane reads of a K row: two QK k-steps each
    static constexpr int DB = D / 16;            // PV d-blocks of 16 rows, read in pairs
    static constexpr int RB = D;                 // K row bytes
    static constexpr int KBYTES = SG * 32 * RB;  // K per stage
    static constexpr int VBYTES = SG * 32 * D;   // V^T per stage
    static constexpr int KCH = KBYTES / 16, VCH = VBYTES / 16;
    static constexpr int STAGE = KBYTES + VBYTES;
    static_assert(D == 64 || D == 128, "fp8 cache: d in {64, 128}");
    static_assert(KCH % 64 == 0 && VCH % 64 == 0 && (KCH / SG) % 64 == 0 && (VCH / SG) % 64 == 0, "whole KiB LDS-DMA pieces");
    typedef MaskedStager<WAVES, KCH, VCH, KBYTES, VBYTES, SG> Stager;
    __device__ __forceinline__ static void offsets(Stager& stg, int wave, int lane) {
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
    }
};

// ---------------------------------------------------------------------------------------
// A prefill item: unit block qb0 of sequence b's K/V slice kvh.  qmha_fp8_band.hip's body over geo = of(L) at Nq = nq_b,
// the sequence's first row r0 in place of b Nq.
// ---------------------------------------------------------------------------------------
template <class Geo, int D>
__device__ __forceinline__ void prefill_item(const float* __restrict__ Qf, const uint8_t* __restrict__ K8, const uint8_t* __restrict__ Vt8,
                                             float* __restrict__ O, const Geo& geo, const Step& sp, char (*lds)[Tiles<D>::STAGE], int b, int kvh,
                                             int qb0, int r0, int H, int d_model, float q_scale, float s_log2, float v_scale) {
    typedef Tiles<D> T;
    constexpr int WAVES = T::WAVES, SG = T::SG, KP = T::KP, DB = T::DB, RB = T::RB, KBYTES = T::KBYTES;
    asm volatile("" : "+v"(s_log2));  // a VOP3 fma reading an SGPR issues at the slow rate
    const int Nk = geo.nk();
    const int U = geo.units();
    const int bh = b * H + kvh;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int u = qb0 * WAVES + wave;
    const bool active = u < U;
    const int qg = geo.group(u), k = geo.head(kvh, u);  // query group, query head
    const int grp = lane >> 4, r16 = lane & 15;
    const int wg_last = geo.last(geo.group(min(qb0 * WAVES + WAVES - 1, U - 1)));     // of the last active wave
    const int t0 = band_first(sp.window, geo.diag(geo.group(qb0 * WAVES))) & ~(SG - 1);  // of the first: the first stage's first tile
    const int nst = (wg_last - t0) / SG + 1;                                           // stages from t0; wg_last >= t0
    const int my_diag = geo.diag(qg);
    const int my_first = band_first(sp.window, my_diag);
    const int my_last = active ? geo.last(qg) : -1;
    // tiles t <= my_left hold a key the group's last row does not see: they take the left select
    const int my_left = (QMHA_GROUP * my_diag + QMHA_GROUP - 1 - sp.window) >> 5;  // floor: negative where there is none

    // Q into the QK B operand: query 16 qb + r16, bytes d = 64 kp + 16 grp + 8 h .. +7 for k-step 2 kp + h
    fp8x8 qop[2][2 * KP];
#pragma unroll
    for (int qb = 0; qb < 2; ++qb)
#pragma unroll
        for (int ks = 0; ks < 2 * KP; ++ks) {
            float x[8] = {};
            if (active && row_real(geo, qg * QMHA_GROUP + 16 * qb + r16)) {  // a pad lane loads nothing
                const float* qp = Qf + ((size_t)r0 + (size_t)qg * QMHA_GROUP + 16 * qb + r16 - row_shift(geo)) * d_model + (size_t)k * D +
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
    // mb: the running maximum less the bias of 8 (log2 units); no score is below -1e30.  l: over this lane's keys
    float mb[2] = {-1e30f, -1e30f}, l_run[2] = {0.0f, 0.0f};

    const char* kbase = reinterpret_cast<const char*>(K8 + (size_t)bh * Nk * D);
    const char* vbase = reinterpret_cast<const char*>(Vt8 + (size_t)bh * Nk * D);
    typename T::Stager stg;
    T::offsets(stg, wave, lane);
    // stage st of the workgroup is stage t0 / 2 + st of the sequence (t0 is even).  Paged: the walk starts at t0, whose
    // column and every later one up to L's passed used_pages_ok (t0 >= t0_min).  Only tiles <= wg_last come in.
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
            const int hid = (QMHA_GROUP * (my_diag - t) - sp.window) + (int)(threadIdx.x & 15);
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
        const float sink = sp.sinks ? sp.sinks[k] * kLog2e : 0.0f;  // k: a real head
#pragma unroll
        for (int qb = 0; qb < 2; ++qb) {
            float l = l_run[qb];
            l += __shfl_xor(l, 16);
            l += __shfl_xor(l, 32);
            // the sink's column: 2^(sink log2(e) - m + 8), mb = m - 8; the exponent clamped, so finite for every finite sink
            if (sp.sinks) l += __builtin_amdgcn_exp2f(fminf(sink - mb[qb], 120.0f));
            const bool ok = l > 1e-10f;  // the fp16 epilogue's guard
            float* orow = O + ((size_t)r0 + (size_t)qg * QMHA_GROUP + 16 * qb + r16 - row_shift(geo)) * d_model + (size_t)k * D + 4 * grp;
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
// A decode item: chunk c of sequence b's K/V slice kvh, a valid sequence of nq rows at r0 with G nq <= 16 QB columns.
// qmha_fp8_decode_window.hip's body; `direct` (workgroup-uniform: the shipped call's one-chunk form) is its DIRECT.
// ---------------------------------------------------------------------------------------
template <class Geo, int D, int QB>
__device__ __forceinline__ void decode_item(const float* __restrict__ Qf, const uint8_t* __restrict__ K8, const uint8_t* __restrict__ Vt8,
                                            float* __restrict__ O, const Geo& any, const Step& sp, char (*lds)[Tiles<D>::STAGE], int b, int kvh,
                                            int c, int r0, int Nq, int L, int t0, bool direct, int H, int d_model, float q_scale, float s_log2,
                                            float v_scale) {
    typedef Tiles<D> T;
    static_assert(kWaves == 4 && kSG == 2, "wave w is (tile w & 1 of the stage, d-half w >> 1)");
    constexpr int WAVES = T::WAVES, SG = T::SG, KP = T::KP, DB = T::DB, RB = T::RB, KBYTES = T::KBYTES;
    constexpr int MH = DB / 2;  // the d-blocks of a wave: dh MH .. +MH - 1
    // the hand-over of a tp = 1 wave at the chunk's end: MH QB v4f of o and QB (m, l) pairs per lane, lane-interleaved
    constexpr int HAND = 64 * (MH * QB * 16 + QB * 8);
    static_assert(2 * HAND <= 2 * T::STAGE, "the hand-over fits the stage buffers");
    const int G = any.G, bh = b * H + kvh;
    const int t_first = t0 + c * sp.C, t_last = (L - 1) / QMHA_GROUP;
    if (t_first > t_last) return;
    const int t_end = min(t_first + sp.C - 1, t_last);  // the chunk's last tile: t_end / 2 < cap / 64
    asm volatile("" : "+v"(s_log2));  // a VOP3 fma reading an SGPR issues at the slow rate

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
        lolim[qb] = lim[qb] - sp.window;  // >= -INT_MAX
    }
    // Q into the QK B operand: column 16 qb + r16, bytes d = 64 kp + 16 grp + 8 h .. +7 for k-step 2 kp + h
    fp8x8 qop[QB][2 * KP];
#pragma unroll
    for (int qb = 0; qb < QB; ++qb)
#pragma unroll
        for (int ks = 0; ks < 2 * KP; ++ks) {
            float x[8] = {};
            if (real[qb]) {  // a pad column loads nothing
                const float* qp = Qf + ((size_t)r0 + row[qb]) * d_model + (size_t)head[qb] * D + 64 * (ks >> 1) + 16 * grp + 8 * (ks & 1);
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
    typename T::Stager stg;
    T::offsets(stg, wave, lane);
    // stage st of the chunk is stage t_first / 2 + st of the sequence (t_first is even: t0 and C are).  Paged: the walk
    // starts at the chunk's first tile, whose column and every later one up to L's passed used_pages_ok.
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
        if (32 * t <= L - 1 - sp.window) {  // wave-uniform: the tile holds a key some column sees no more
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
        // the shipped kernel's contractions, spelled out: which product of a sum of two is fused decides the last bit
        const float l = fmaf(w0, l_run[qb], w1 * ml[1]);
        if (direct) {
            // the only chunk: every real row has its own key e_r in it.  The sink joins the row sum, then O itself
            if (!real[qb]) continue;
            const float lt = sp.sinks ? l + sink_term(sp.sinks[head[qb]], M) : l;
            const bool ok = lt > 1e-10f;
            float* orow = O + ((size_t)r0 + row[qb]) * d_model + (size_t)head[qb] * D + 16 * (dh * MH) + 4 * grp;
#pragma unroll
            for (int m = 0; m < MH; ++m) {
                const v4f o1 = *reinterpret_cast<const v4f*>(hand + ((m * QB + qb) * 64 + lane) * 16);
                v4f w;
#pragma unroll
                for (int j = 0; j < 4; ++j) w[j] = ok ? v_scale * (fmaf(w1, o1[j], w0 * o[m][qb][j]) / lt) : 0.0f;
                *reinterpret_cast<v4f*>(orow + 16 * m) = w;
            }
        } else {
            const bool ok = l > 1e-10f;  // false: no key of the chunk is visible to the row -- l = 0, Oc = 0, m = -1e30 + 8
            // row r writes chunk c iff c <= ((L - Nq + r) / 32 - t0) / C: what the combine reads of it
            if (!real[qb] || c > (lim[qb] / QMHA_GROUP - t0) / sp.C) continue;
            const size_t at = ((size_t)b * sp.NC + c) * sp.RQ + row[qb];  // row < Nq <= RQ
            float* orow = sp.Oc + at * d_model + (size_t)head[qb] * D + 16 * (dh * MH) + 4 * grp;
#pragma unroll
            for (int m = 0; m < MH; ++m) {
                const v4f o1 = *reinterpret_cast<const v4f*>(hand + ((m * QB + qb) * 64 + lane) * 16);
                v4f w;
#pragma unroll
                for (int j = 0; j < 4; ++j) w[j] = ok ? v_scale * (fmaf(w1, o1[j], w0 * o[m][qb][j]) / l) : 0.0f;
                *reinterpret_cast<v4f*>(orow + 16 * m) = w;
            }
            if (dh == 0 && grp == 0) {
                sp.pl[at * h + head[qb]] = l;
                sp.pm[at * h + head[qb]] = M + 8.0f;  // the true maximum
            }
        }
    }
}

}  // namespace mixed

// (the launch bound of the two bodies it holds: four waves per SIMD at d = 64, two at d = 128; no scratch memory)
template <class Geo, int D>
__global__ __launch_bounds__(kWaves * 64, D > 64 ? 2 : 4) void qmha_fp8_mixed_kernel(
    const float* __restrict__ Qf, const uint8_t* __restrict__ K8, const uint8_t* __restrict__ Vt8, float* __restrict__ O, Geo any, mixed::Step sp,
    const int32_t* __restrict__ lens, int H, int d_model, float q_scale, float s_log2, float v_scale) {
    static_assert(kRaggedGeo<Geo> && !kSplitGeo<Geo> && !kPackedGeo<Geo> && !kWindowGeo<Geo>, "Ragged or Paged");
    __shared__ __attribute__((aligned(16))) char lds[2][mixed::Tiles<D>::STAGE];
    const int G = any.G, cap = any.Nk;
    const int npre = H * sp.PB;
    if ((int)blockIdx.x < npre) {
        // a prefill item: every wave locates (b, block) from the same words, before any barrier or DMA issue
        const int kvh = blockIdx.x / sp.PB, idx = blockIdx.x % sp.PB;
        int b = 0, blk = 0;
        const bool found = mixed::locate(sp.B, idx, [&](int s) {
            int r0, nq;
            if (!mixed::seq_rows(sp, s, r0, nq) || (long long)G * nq <= 32) return 0;
            const int L = lens[s];
            if (L < nq || L > cap) return 1;
            const long long units = (long long)G * ((((L - nq) & (QMHA_GROUP - 1)) + (long long)nq + QMHA_GROUP - 1) / QMHA_GROUP);
            const long long blocks = (units + kWaves - 1) / kWaves;
            return blocks < sp.PB ? (int)blocks : sp.PB;
        }, b, blk);
        if (!found) return;
        b = __builtin_amdgcn_readfirstlane(b), blk = __builtin_amdgcn_readfirstlane(blk);
        const int r0 = __builtin_amdgcn_readfirstlane(sp.cu[b]), nq = __builtin_amdgcn_readfirstlane(sp.cu[b + 1]) - r0;  // in range: count_b > 0
        const int L = __builtin_amdgcn_readfirstlane(lens[b]);
        Geo seq = any;
        seq.Nq = nq;
        bool valid = seq.valid(L);
        const Geo geo = seq.of(valid ? L : nq);
        if constexpr (kPagedGeo<Geo>) {
            if (valid) valid = seq.used_pages_ok(b, QMHA_GROUP * (mixed::band_first(sp.window, geo.diag(0)) & ~(kSG - 1)), L);
        }
        if (!valid) {  // the sequence's rows of O are zeros, written by block 0 of each K/V head; none of its K/V is read
            if (blk == 0) mixed::zero_rows<D>(O, r0, nq, G, kvh, d_model);
            return;
        }
        const int nqb = (geo.units() + kWaves - 1) / kWaves;  // count_b: blk < nqb
        if (blk >= nqb) return;
        mixed::prefill_item<Geo, D>(Qf, K8, Vt8, O, geo, sp, lds, b, kvh, nqb - 1 - blk, r0, H, d_model, q_scale, s_log2, v_scale);
        return;
    }
    // a decode item (b, kvh, c): the sequence's words, its kind and its verdict, workgroup-uniform
    const unsigned it = blockIdx.x - npre;
    const int c = (int)(it % (unsigned)sp.NC), bh = (int)(it / (unsigned)sp.NC);
    const int b = bh / H, kvh = bh % H;
    if (b >= sp.B) return;
    const int r0 = __builtin_amdgcn_readfirstlane(sp.cu[b]), r1 = __builtin_amdgcn_readfirstlane(sp.cu[b + 1]);
    if (r0 < 0 || r1 <= r0 || r1 > sp.total) return;  // the range never becomes an address; an empty sequence sits out
    const int nq = r1 - r0;
    if ((long long)G * nq > 32) return;  // the prefill kind
    const int nc = mixed::window_chunks(cap, nq, sp.window, sp.C);  // the chunks of the shipped call at Nq = nq
    if (c >= nc) return;
    const bool direct = nc == 1;
    const int L = __builtin_amdgcn_readfirstlane(lens[b]);
    bool valid = L >= nq && L <= cap;
    const int t0 = valid ? mixed::window_t0(L, nq, sp.window) : 0;
    if constexpr (kPagedGeo<Geo>) {
        if (valid) valid = any.used_pages_ok(b, t0 * QMHA_GROUP, L);
    }
    if (!valid) {  // the combine form's zeros are the combine kernel's
        if (direct) mixed::zero_rows<D>(O, r0, nq, G, kvh, d_model);
        return;
    }
    if (G * nq > 16)
        mixed::decode_item<Geo, D, 2>(Qf, K8, Vt8, O, any, sp, lds, b, kvh, c, r0, nq, L, t0, direct, H, d_model, q_scale, s_log2, v_scale);
    else
        mixed::decode_item<Geo, D, 1>(Qf, K8, Vt8, O, any, sp, lds, b, kvh, c, r0, nq, L, t0, direct, H, d_model, q_scale, s_log2, v_scale);
}

// The combine pass of the decode kind: a thread per 16 bytes of a row of a sequence's widest query block (32 / G rows),
// qmha_fp8_decode_window_combine_kernel's arithmetic in its order.  Everything but a decode-kind sequence in range whose
// shipped call has more than one chunk is skipped; an invalid one of those gets positive zeros, no scratch read.
__global__ __launch_bounds__(256) void qmha_fp8_mixed_combine_kernel(Paged any, mixed::Step sp, float* __restrict__ O,
                                                                     const int32_t* __restrict__ lens, int h, int D, float thr) {
    const int W4 = h * D / 4;  // 16-byte pieces of a row
    const unsigned per = ((unsigned)sp.RQ * (unsigned)W4 + 255u) / 256u;  // blocks of a sequence
    const int b = (int)(blockIdx.x / per);
    if (b >= sp.B) return;
    const int r0 = sp.cu[b], r1 = sp.cu[b + 1];
    if (r0 < 0 || r1 <= r0 || r1 > sp.total) return;
    const int nq = r1 - r0;
    if ((long long)any.G * nq > 32 || mixed::window_chunks(any.Nk, nq, sp.window, sp.C) == 1) return;
    const int L = lens[b];
    bool valid = L >= nq && L <= any.Nk;
    const int t0 = valid ? mixed::window_t0(L, nq, sp.window) : 0;
    if (valid && any.table) valid = any.used_pages_ok(b, t0 * QMHA_GROUP, L);  // block-uniform: every lane takes part in the ballot
    const int i = (int)(blockIdx.x % per) * 256 + threadIdx.x;
    if (i >= nq * W4) return;
    const int r = i / W4, w = i % W4, k = w / (D / 4);
    float* o = O + ((size_t)r0 + r) * ((size_t)h * D) + 4 * w;
    if (!valid) {
        *reinterpret_cast<v4f*>(o) = v4f{};
        return;
    }
    const int n = ((L - nq + r) / QMHA_GROUP - t0) / sp.C + 1;  // <= nc_b <= NC
    const size_t step = (size_t)sp.RQ * h, at = ((size_t)b * sp.NC * sp.RQ + r) * h + k;  // chunk c: at + c step
    float M = sp.pm[at];
    for (int c = 1; c < n; ++c) M = fmaxf(M, sp.pm[at + c * step]);
    float Ltot = 0.0f;
    v4f acc = v4f{};
    for (int c = 0; c < n; ++c) {
        const float a = sp.pl[at + c * step] * __builtin_amdgcn_exp2f(sp.pm[at + c * step] - M);
        const v4f oc = *reinterpret_cast<const v4f*>(sp.Oc + (((size_t)b * sp.NC + c) * sp.RQ + r) * ((size_t)h * D) + 4 * w);
        Ltot += a;
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] = fmaf(a, oc[e], acc[e]);
    }
    if (sp.sinks) Ltot += mixed::sink_term(sp.sinks[k], M - 8.0f);
    v4f res;
#pragma unroll
    for (int e = 0; e < 4; ++e) res[e] = Ltot > thr ? acc[e] / Ltot : 0.0f;
    *reinterpret_cast<v4f*>(o) = res;
}

// ---------------------------------------------------------------------------------------
// The append.  Dst: where group g of a K/V slice lies -- qmha_kv_fp8.hip's SliceRows / PoolRows restated
// ---------------------------------------------------------------------------------------
namespace mixed {

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
    // every entry of the pages that groups g0 .. g1 of sequence b touch lies in the pool (lanes take the columns)
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
__device__ __forceinline__ uint32_t pack4(const float (&x)[4], float scale) {
    float y[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) y[c] = fminf(fmaxf(x[c] / scale, -448.0f), 448.0f);
    int w = 0;
    w = __builtin_amdgcn_cvt_pk_fp8_f32(y[0], y[1], w, false);
    w = __builtin_amdgcn_cvt_pk_fp8_f32(y[2], y[3], w, true);
    return (uint32_t)w;
}

}  // namespace mixed

// One wave per (tensor: blockIdx.y, K/V head, item i < AB), AB = mixed_append_groups(total, B) >= the groups all sequences
// touch: n rows at p touch groups p / 32 .. (p + n - 1) / 32, at most n / 32 + 2.  count_b: 0 for an empty or out-of-range
// sequence (pos[b] is not read) or a pos[b] outside [0, cap - n_b]; else the groups touched.
template <class Dst, int D>
__global__ __launch_bounds__(256) void qmha_fp8_mixed_rows_kernel(const float* __restrict__ K, const float* __restrict__ V, uint8_t* __restrict__ K8,
                                                                  uint8_t* __restrict__ Vt8, const int32_t* __restrict__ cu,
                                                                  const int32_t* __restrict__ pos, Dst dst, int B, int rows, int H, int d_model,
                                                                  int AB, float k_scale, float v_scale) {
    const int lane = threadIdx.x & 63;
    const int item = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));  // (K/V head, i)
    if (item >= H * AB) return;  // per wave; no workgroup barrier follows
    const int kh = item / AB, idx = item % AB;
    const mixed::Step sp{cu, rows, B};
    int b = 0, j = 0;
    const bool found = mixed::locate(B, idx, [&](int s) {
        int r0, n;
        if (!mixed::seq_rows(sp, s, r0, n)) return 0;
        const int p = pos[s];
        if (p < 0 || p > dst.capacity() - n) return 0;  // an invalid row: the sequence writes nothing
        return min((p + n - 1) / QMHA_GROUP - p / QMHA_GROUP + 1, AB);
    }, b, j);
    if (!found) return;
    b = __builtin_amdgcn_readfirstlane(b), j = __builtin_amdgcn_readfirstlane(j);
    const int r0 = __builtin_amdgcn_readfirstlane(cu[b]), n = __builtin_amdgcn_readfirstlane(cu[b + 1]) - r0;  // in range: count_b > 0
    const int p = __builtin_amdgcn_readfirstlane(pos[b]);
    const int g0 = p / QMHA_GROUP, g1 = (p + n - 1) / QMHA_GROUP, g = g0 + j;
    if (g > g1 || !dst.ok(b, g0, g1)) return;
    const size_t gi = dst.group(b, kh, H, g);
    const int lo = p - g * QMHA_GROUP, hi = lo + n;  // the new rows of this group: lo <= r < hi
    const bool opens = lo <= 0;                      // else rows [0, lo) are earlier appends' and stay
    const float* src = (blockIdx.y ? V : K) + ((ptrdiff_t)r0 - lo) * d_model + (ptrdiff_t)kh * D;  // row r of the group: src + r * d_model
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
            *reinterpret_cast<uint32_t*>(out + (size_t)r * D) = mixed::pack4(x, k_scale);
        }
        return;
    }
    uint8_t* blk = Vt8 + gi * (size_t)(QMHA_GROUP * D);
#pragma unroll 2
    for (int e = lane; e < D * 8; e += 64) {  // dword (d, a): key rows 4 a .. 4 a + 3 of V^T row d
        const int d = e % D, q0 = 4 * (e / D);
        if (q0 + 4 <= lo || (q0 >= hi && !opens)) continue;
        float x[4] = {};
#pragma unroll
        for (int c = 0; c < 4; ++c)
            if (q0 + c >= lo && q0 + c < hi) x[c] = src[(ptrdiff_t)(q0 + c) * d_model + d];
        uint32_t w = mixed::pack4(x, v_scale);
        uint32_t* out = reinterpret_cast<uint32_t*>(blk + fp8_vt_offset(d, q0));
        if (q0 < lo) {  // lo > 0: the group stays open, bytes of rows q0 .. lo - 1 are kept
            const uint32_t keep = (1u << (8 * (lo - q0))) - 1u;
            w = (w & ~keep) | (*out & keep);
        }
        *out = w;
    }
}

// ---------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------
template <class Geo>
static hipError_t fp8_mixed_launch(const Fp8Workspace& w, const float* Qf, float* O, const MaskedCall& c, const int32_t* cu, int total, int window,
                                   const float* sinks, int chunk_rows, void* scratch, hipStream_t stream, Geo geo) {
    const int G = c.H / c.Hkv, RQ = mixed_rows(G), NC = mixed_chunks(c.Nk, G, window, chunk_rows);
    const long long PB = mixed_prefill_blocks(total, c.B, G), grid_n = (long long)c.Hkv * PB + (long long)c.B * c.Hkv * NC;
    if (PB * 65 > INT_MAX || grid_n > INT_MAX || ((long long)RQ * c.d_model / 4 + 255) / 256 * c.B > INT_MAX) return hipErrorInvalidValue;
    const SplitScratch s = split_carve(scratch, c.B, NC, RQ, c.H, c.D);
    const mixed::Step sp{cu, total, c.B, window, sinks, s.Oc, s.m, s.l, chunk_rows / QMHA_GROUP, NC, RQ, (int)PB};
    const hipError_t e = fp8_cache_d(c.D, [&](auto d) {
        hipLaunchKernelGGL((qmha_fp8_mixed_kernel<Geo, decltype(d)::value>), dim3((unsigned)grid_n), dim3(kWaves * 64), 0, stream, Qf, w.K8, w.Vt8, O,
                           geo, sp, c.lens, c.Hkv, c.d_model, w.q_scale, w.q_scale * w.k_scale * softmax_scale_log2(c.D), w.v_scale);
        return hipGetLastError();
    });
    if (e != hipSuccess || NC == 1) return e;
    const dim3 cgrid((unsigned)(((size_t)RQ * c.d_model / 4 + 255) / 256 * c.B));
    hipLaunchKernelGGL(qmha_fp8_mixed_combine_kernel, cgrid, dim3(256), 0, stream, as_paged(geo), sp, O, c.lens, c.H, c.D, 1e-10f);
    return hipGetLastError();
}

hipError_t launch_fp8_mixed(const Fp8Workspace& w, const float* Qf, float* O, const MaskedCall& c, const int32_t* cu, int total, int window,
                            const float* sinks, int chunk_rows, void* scratch, hipStream_t stream) {
    if (!c.ragged || !cu || !scratch || total < 1 || window < 1 || chunk_rows < 2 * QMHA_GROUP || chunk_rows % (2 * QMHA_GROUP) != 0 ||
        chunk_rows > c.Nk)
        return hipErrorInvalidValue;
    return masked_geo(c, [&](auto geo) {
        if constexpr (kRaggedGeo<decltype(geo)>) return fp8_mixed_launch(w, Qf, O, c, cu, total, window, sinks, chunk_rows, scratch, stream, geo);
        else return hipErrorInvalidValue;
    });
}

template <class Dst>
static hipError_t kv_mixed_launch(const float* K, const float* V, const Fp8Workspace& w, int B, int total, const int32_t* cu, const int32_t* pos,
                                  Dst dst, int H, int D, int d_model, hipStream_t stream) {
    const long long AB = mixed_append_groups(total, B);
    if (AB * 65 > INT_MAX || AB * H > INT_MAX) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((AB * H + 3) / 4), 2);
    return fp8_cache_d(D, [&](auto d) {
        hipLaunchKernelGGL((qmha_fp8_mixed_rows_kernel<Dst, decltype(d)::value>), grid, dim3(256), 0, stream, K, V, w.K8, w.Vt8, cu, pos, dst, B, total,
                           H, d_model, (int)AB, w.k_scale, w.v_scale);
        return hipGetLastError();
    });
}

hipError_t launch_kv_mixed(const float* K, const float* V, const Fp8Workspace& w, int B, int total, int cap, const int32_t* cu, const int32_t* pos,
                           int H, int D, int d_model, hipStream_t stream, const PageTable& pt) {
    if (B < 1 || H < 1 || !cu || !pos || total < 1 || cap < QMHA_GROUP || cap % QMHA_GROUP != 0) return hipErrorInvalidValue;
    if (!pt.table) return kv_mixed_launch(K, V, w, B, total, cu, pos, mixed::SliceRows{cap}, H, D, d_model, stream);
    if (pt.page_rows < 2 * QMHA_GROUP || pt.page_rows % (2 * QMHA_GROUP) != 0 || pt.max_pages < 1 || pt.num_pages < 1 ||
        (long long)pt.max_pages * pt.page_rows != cap)
        return hipErrorInvalidValue;
    return kv_mixed_launch(K, V, w, B, total, cu, pos, mixed::PoolRows{pt.table, pt.page_rows / QMHA_GROUP, pt.max_pages, pt.num_pages}, H, D,
                           d_model, stream);
}

}  // namespace qmha
