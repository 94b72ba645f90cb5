    // qmha_fa_masked_f16.inc -- the body of every fp16 kernel of qmha_fa_masked.hip, included inside the __global__
    // (why a text include and no __device__ function: DESIGN.md 15.3).  In scope: D, the geometry `geo`, and the
    // arguments Qf, Kh, Vt, O, H, d_model, nqb, c_log2.  row_shift(geo) / row_real(geo, row) (qmha_fa_masked.hip) are
    // 0 / true for every geometry but Ragged, whose query rows sit `s` rows into their 32-row groups.  Split<Geo>
    // (DESIGN.md 19): one unit block of one chunk of tiles per workgroup -- tile_first / tile_end bound the sweep,
    // out_base / out_slice send the epilogue's O to the scratch, and the row's l and m are stored beside it.
    // seq_row0(geo, slice): the first row of a sequence in Q / O, slice * Nq but for Packed<Geo> (DESIGN.md 20), whose
    // sequences lie at cu[b] in operands without a batch axis.
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
    constexpr bool SPLIT = kSplitGeo<decltype(geo)>;
    // Window<Geo> (DESIGN.md 22): the sweep starts at the stage of tile_first(geo), a wave computes tiles first(qg) ...
    // last(qg) from the zero state, and tile left(qg) takes the complement of the diagonal's mask
    constexpr bool WINDOW = kWindowGeo<decltype(geo)>;
    int bh, qb0;
    if constexpr (SPLIT) {  // the chunk is geo.c
        int c_;
        split_wg(nqb, geo.NC, bh, qb0, c_);
    } else
    masked_wg_single(nqb, bh, qb0);
    const int b = bh / H, kvh = bh % H;  // bh: the K/V slice (H K/V heads)
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if constexpr (kRaggedGeo<decltype(geo)>) {  // its grid follows the host's Nq, U the sequence's length: a workgroup with
        if (qb0 * WAVES >= U) return;           // no active unit leaves before any barrier or DMA issue
    }
    const int u = qb0 * WAVES + wave;
    const bool active = u < U && (SPLIT ? geo.last(geo.group(u)) >= tile_first(geo) : true);  // Split: the wave reaches the chunk
    const int qg = geo.group(u), k = geo.head(kvh, u);  // query group, query head
    const int grp = lane >> 4, r16 = lane & 15;
    const int wg_last = tile_end(geo, geo.last(geo.group(min(qb0 * WAVES + WAVES - 1, U - 1))));  // of the last active wave
    if constexpr (SPLIT) {  // no unit reaches the chunk: the workgroup leaves before any barrier or DMA issue
        if (wg_last < tile_first(geo)) return;
    }
    const int nst = wg_last / SG + 1, st0 = tile_first(geo) / SG;  // the workgroup runs stages st0 ... nst - 1
    const int my_diag = geo.diag(qg);  // this wave's diagonal tile
    const int my_last = active ? tile_end(geo, geo.last(qg)) : -1;
    int my_first = 0, my_left = -1;  // Window: this wave's first tile and its left tile (negative: none).  Wave-uniform
    if constexpr (WINDOW) my_first = geo.first(qg), my_left = geo.left(qg);

    // Q converted in-kernel (RNE) into the QK B operand: query 16 qb + r16, d = 32 ks + 8 grp .. +7
    v8h qop[2][KS];
#pragma unroll
    for (int qb = 0; qb < 2; ++qb)
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            if (active && row_real(geo, qg * QMHA_GROUP + 16 * qb + r16)) {  // a pad lane (Ragged) loads nothing
                const float* qp = Qf + (seq_row0(geo, b) + (size_t)qg * QMHA_GROUP + 16 * qb + r16 - row_shift(geo)) * d_model + (size_t)k * D +
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
    // Paged: the stage's page slice is the buffer (base formed in 64 bits, records of one page slice), the stage offset
    // the stage's place in its page
    std::conditional_t<kPagedGeo<decltype(geo)>, PageWalk, NoWalk> walk;
    if constexpr (kPagedGeo<decltype(geo)> && WINDOW) walk.start_at(geo, b, tile_first(geo));  // the first stage's first tile
    else
    if constexpr (kPagedGeo<decltype(geo)> && kSplitGeo<decltype(geo)>) walk.start_at(geo, b, tile_first(geo));
    else if constexpr (kPagedGeo<decltype(geo)>) walk.start(geo, b);
    auto issue = [&](int buf, int st) {
        if constexpr (kPagedGeo<decltype(geo)>) {
            walk.take(geo);
            const size_t slice = (size_t)walk.page * H + kvh, pbytes = (size_t)geo.PG * (QMHA_GROUP * RB);
            stg.issue(lds[buf], reinterpret_cast<const char*>(Kh) + slice * pbytes, (int)pbytes,
                      reinterpret_cast<const char*>(Vt) + slice * pbytes, (int)pbytes, walk.sip,
                      min(SG, wg_last + 1 - st * SG), wave);
            walk.advance(geo, b);
        } else
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
    // qmha_fa_f16_v3_kernel; diag: the diagonal tile (Window: and left_tile says the tile is that of the window's left edge)
    bool left_tile = false;
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
        if constexpr (WINDOW) {
            // The complement of the diagonal's select: key c is visible to row r iff c > r.  w >= 1 (window >= 32, checked
            // by the host), so left(qg) = diag(qg) - w < diag(qg): a tile takes one select or the other, never both.
            if (left_tile) {  // wave-uniform
#pragma unroll
                for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                    for (int qb = 0; qb < 2; ++qb)
#pragma unroll
                        for (int i = 0; i < 4; ++i)
                            s.v[kb][qb][i] = key0 + i + 8 * kb <= 16 * qb + r16 ? -__builtin_huge_valf() : s.v[kb][qb][i];
            }
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
                // the query's four lane groups (key 0 is never masked: finite -- but in a window's left tile, where row 31
                // sees no key: its mx is -inf, its ts is 0 in all four lanes, so its `rows` bit is clear and mx goes unused)
                mx = fmaxf(mx, __shfl_xor(mx, 16));
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

    issue(0, st0);
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
                if constexpr (WINDOW) {
                    left_tile = t == my_left;
                    if (t >= my_first && t <= my_last) tile(L, gi, qk(L, gi), t == my_diag);
                } else
                if (t <= my_last) tile(L, gi, qk(L, gi), t == my_diag);
                __builtin_amdgcn_sched_barrier(0);  // one tile's registers at a time
            }
        }
        qmha_dma_barrier();
    };
    int st = st0;
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
            float* orow = out_base(geo, O) + (seq_row0(geo, out_slice(geo, b)) + (size_t)qg * QMHA_GROUP + 16 * qb + r16 - row_shift(geo)) * d_model + (size_t)k * D + 4 * grp;
            if (row_real(geo, qg * QMHA_GROUP + 16 * qb + r16)) {  // a pad lane stores nothing
#pragma unroll
            for (int m = 0; m < DB; ++m) {
                v4f w;
#pragma unroll
                for (int j = 0; j < 4; ++j) w[j] = ok ? o[m][qb][j] / l : 0.0f;
                *reinterpret_cast<v4f*>(orow + 16 * m) = w;
            }
            if constexpr (SPLIT) {  // the chunk's l and m of a real row, [B][NC][Nq][h]: what the combine weighs Oc with
                if (grp == 0) {
                    const size_t i = ((size_t)out_slice(geo, b) * Nq + (size_t)(qg * QMHA_GROUP + 16 * qb + r16 - row_shift(geo))) * (size_t)(H * geo.G) + k;
                    geo.pl[i] = l;
                    geo.pm[i] = m_run[qb];
                }
            }
            }
        }
    }
