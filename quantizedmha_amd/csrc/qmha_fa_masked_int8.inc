    // qmha_fa_masked_int8.inc -- the body of every int8 kernel of qmha_fa_masked.hip, included inside the __global__
    // (why a text include and no __device__ function: DESIGN.md 15.3).  In scope: D, Geo, the geometry `geo`, and the
    // arguments Qf, Ki, Vh, sK, sV, O, H, d_model, nqb, c_log2.  row_shift(geo) / row_real(geo, row) (qmha_fa_masked.hip)
    // are 0 / true for every geometry but Ragged, whose query rows sit `s` rows into their 32-row groups.  Split<Geo>
    // (DESIGN.md 19): one unit block of one chunk of tiles per workgroup -- tile_first / tile_end bound the sweep,
    // out_base / out_slice send the epilogue's O to the scratch, and the row's l and m are stored beside it.
    // Packed<Geo> (DESIGN.md 20): the first row of a sequence in Q / O is seq_row0(geo, b) = cu[b], where every other
    // geometry has b * Nq; under `if constexpr`, so the other instances' IR is what it was.
    constexpr int WAVES = kWaves, SG = kSG;
    constexpr int KS = D / 32;               // i8 MFMA k-steps (QK) and d-blocks (PV)
    constexpr int KBYTES = SG * 32 * D;      // K int8 per stage
    constexpr int VBYTES = SG * 32 * D * 2;  // V f16 per stage
    constexpr int KCH = KBYTES / 16, VCH = VBYTES / 16;
    constexpr bool DUMP = Geo::kDump;  // also store what the kernel computed (Dumping<Geo>), per tile a wave runs
    constexpr bool SPLIT = kSplitGeo<decltype(geo)>;
    // Window<Geo> (DESIGN.md 22): one unit block per workgroup; the sweep starts at the stage of tile_first(geo), a wave
    // computes tiles first(qg) ... last(qg) from the zero state, and tile left(qg) takes the complement of the diagonal's mask
    constexpr bool WINDOW = kWindowGeo<decltype(geo)>;
    static_assert(D == 32 || D == 64 || D == 128, "masked int8: d in {32, 64, 128}");
    static_assert(KCH % 64 == 0 && VCH % 64 == 0 && (KCH / SG) % 64 == 0, "whole KiB LDS-DMA pieces");
    __shared__ __attribute__((aligned(16))) char lds[2][KBYTES + VBYTES];

    const int Nq = geo.nq(), Nk = geo.nk();
    const int Gq = Nq / QMHA_GROUP, Gk = geo.gk(), U = geo.units();
    int bh, pi;
    if constexpr (SPLIT) {  // no pair: a chunk has no triangle to balance; pi is the unit block, the chunk is geo.c
        int c_;
        split_wg(nqb, geo.NC, bh, pi, c_);
    } else
    if constexpr (WINDOW) masked_wg_single(nqb, bh, pi);  // no pair either: a band has no triangle; pi is the unit block
    else
    masked_wg(nqb, bh, pi);
    const int b = bh / H, kvh = bh % H;  // bh: the K/V slice (H K/V heads)
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int half = lane >> 5, col = lane & 31;
#pragma nounroll
    for (int pass = 0; pass < 2; ++pass) {  // the pair's large q-block, then its mirror (uniform)
    const int qb = (SPLIT || WINDOW) ? pi : pass == 0 ? nqb - 1 - pi : pi;
    if (pass == 1 && (SPLIT || WINDOW || pi == nqb - 1 - pi)) break;  // odd nqb: the middle q-block has no partner
    if constexpr (kRaggedGeo<decltype(geo)>) {  // its grid follows the host's Nq, U the sequence's length: a pass with no
        if (qb * WAVES >= U) continue;          // active unit leaves before any barrier or DMA issue (workgroup-uniform)
    }
    const int u = qb * WAVES + wave;
    // wave-uniform; an inactive wave still stages and syncs.  Split: so does a wave whose tiles end before the chunk
    const bool active = u < U && (SPLIT ? geo.last(geo.group(u)) >= tile_first(geo) : true);
    const int qg = geo.group(u), k = geo.head(kvh, u);  // query group, query head
    // the workgroup's last tile: that of its last active wave
    const int wg_last = tile_end(geo, geo.last(geo.group(min(qb * WAVES + WAVES - 1, U - 1))));
    if constexpr (SPLIT) {  // no unit reaches the chunk: the workgroup leaves before any barrier or DMA issue
        if (wg_last < tile_first(geo)) break;
    }
    const int nst = wg_last / SG + 1, st0 = tile_first(geo) / SG;  // the pass runs stages st0 ... nst - 1
    const int my_diag = geo.diag(qg);              // this wave's diagonal tile
    const int my_last = active ? tile_end(geo, geo.last(qg)) : -1;  // this wave computes tiles t <= my_last
    int my_first = 0, my_left = -1;  // Window: ... and t >= my_first; its left tile (negative: none).  Wave-uniform
    if constexpr (WINDOW) my_first = geo.first(qg), my_left = geo.left(qg);

    // in-register Q quantisation (fa_tc_int8_b.cu:33-152) into the Q^T operand: lane (col, half) holds
    // bytes [32 s + 16 half, +16) of query row col for every k-step s
    v4i qop[KS];
    float cq = 0.0f;
    if (active) {
        const float* qrow = Qf + ((size_t)b * Nq + (size_t)qg * QMHA_GROUP + col) * d_model + (size_t)k * D;
        if constexpr (kPackedGeo<decltype(geo)>) qrow = Qf + (seq_row0(geo, b) + (size_t)qg * QMHA_GROUP + col) * d_model + (size_t)k * D;
        if constexpr (kRaggedGeo<decltype(geo)>) qrow -= (size_t)row_shift(geo) * d_model;
        v4f x[KS][4];
        float amax = 0.0f;
#pragma unroll
        for (int s = 0; s < KS; ++s)
#pragma unroll
            for (int c4 = 0; c4 < 4; ++c4) {
                if constexpr (kRaggedGeo<decltype(geo)>) {  // a pad lane holds a zero row and loads nothing
                    x[s][c4] = v4f{};
                    if (row_real(geo, qg * QMHA_GROUP + col)) x[s][c4] = *reinterpret_cast<const v4f*>(qrow + 32 * s + 16 * half + 4 * c4);
                } else
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
    if constexpr (kPagedGeo<decltype(geo)>) skb = sK, svb = sV;  // bh is no slice of a pool: set per stage, below

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
    // Paged: the stage's page slice is the buffer (base formed in 64 bits, records of one page slice), the stage offset
    // the stage's place in its page; skb / svb follow the page a stage was issued with (the head of `stage` below)
    std::conditional_t<kPagedGeo<decltype(geo)>, PageWalk, NoWalk> walk;
    if constexpr (kPagedGeo<decltype(geo)> && WINDOW) walk.start_at(geo, b, tile_first(geo));  // the first stage's first tile
    else
    if constexpr (kPagedGeo<decltype(geo)> && kSplitGeo<decltype(geo)>) walk.start_at(geo, b, tile_first(geo));
    else if constexpr (kPagedGeo<decltype(geo)>) walk.start(geo, b);
    auto issue = [&](int buf, int st) {
        if constexpr (kPagedGeo<decltype(geo)>) {
            walk.take(geo);
            const size_t slice = (size_t)walk.page * H + kvh, pbytes = (size_t)geo.PG * (QMHA_GROUP * D);
            stg.issue(lds[buf], reinterpret_cast<const char*>(Ki) + slice * pbytes, (int)pbytes,
                      reinterpret_cast<const char*>(Vh) + slice * (2 * pbytes), (int)(2 * pbytes), walk.sip,
                      min(SG, wg_last + 1 - st * SG), wave);
            walk.advance(geo, b);
        } else
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
    // diag: the diagonal tile (Window: and t == my_left is the tile of the window's left edge)
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
        if constexpr (WINDOW) {
            // The complement of the diagonal's select: key c is visible to row r iff c > r.  w >= 1 (window >= 32, checked
            // by the host), so left(qg) = diag(qg) - w < diag(qg): a tile takes one select or the other, never both.
            if (t == my_left) {  // wave-uniform
#pragma unroll
                for (int r = 0; r < 16; ++r) sf[r] = acc_row(r, 0) <= mask_col ? -__builtin_huge_valf() : sf[r];
            }
        }
        float mx = fmaxf(fmaxf(sf[0], sf[1]), sf[2]);
#pragma unroll
        for (int r = 3; r < 15; r += 2) mx = fmaxf(fmaxf(mx, sf[r]), sf[r + 1]);
        // finite: key 0 of the tile is never masked -- but in a window's left tile, where key 0 is always masked and row 31
        // sees nothing: mx = -inf, mx * c = -inf (c > 0), m_new = m_run (finite from m0 = 0), every p of the row is
        // exp2(-inf) = 0, and pmax comes from the rows that see a key (row 30 always does).  No NaN is formed.
        mx = half_swap_max(fmaxf(mx, sf[15]));
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

    issue(0, st0);
    qmha_dma_barrier();  // waits vmcnt(0): stage st0 has landed
    auto stage = [&](auto BUF, int st) {
        constexpr int buf = decltype(BUF)::value;
        if constexpr (kPagedGeo<decltype(geo)>) {  // the scales of the page this stage was issued with: skb[t] is its group t - tile0
            const ptrdiff_t g0 = ((ptrdiff_t)walk.page * H + kvh) * geo.PG - walk.tile0;
            skb = sK + g0, svb = sV + g0;
        }
        if (st + 1 < nst) issue(buf ^ 1, st + 1);  // buf^1 was released by the previous barrier
        const int t0 = st * SG;
        if (t0 <= my_last) {  // wave-uniform
            const char* L = lds[buf];
#pragma unroll
            for (int gi = 0; gi < SG; ++gi) {
                const int t = t0 + gi;
                if constexpr (WINDOW) {
                    if (t >= my_first && t <= my_last) tile(L, gi, t, qk(L, gi), t == my_diag);
                } else
                if (t <= my_last) tile(L, gi, t, qk(L, gi), t == my_diag);
                __builtin_amdgcn_sched_barrier(0);  // one tile's registers at a time
            }
        }
        qmha_dma_barrier();  // vmcnt(0) + barrier: stage st+1 landed, stage st released
    };
    int st = st0;
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
        float* orow = out_base(geo, O) + ((size_t)out_slice(geo, b) * Nq + (size_t)qg * QMHA_GROUP + col) * d_model + (size_t)k * D + 4 * half;
        if constexpr (kPackedGeo<decltype(geo)>) orow = O + (seq_row0(geo, b) + (size_t)qg * QMHA_GROUP + col) * d_model + (size_t)k * D + 4 * half;
        if constexpr (kRaggedGeo<decltype(geo)>) orow -= (size_t)row_shift(geo) * d_model;
        if (kRaggedGeo<decltype(geo)> ? row_real(geo, qg * QMHA_GROUP + col) : true)  // a pad lane (Ragged) stores nothing
#pragma unroll
        for (int m = 0; m < KS; ++m)
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) {
                v4f w;
#pragma unroll
                for (int jj = 0; jj < 4; ++jj) w[jj] = ok ? (o[m][4 * g4 + jj] * unanchor) / l : 0.0f;
                *reinterpret_cast<v4f*>(orow + 32 * m + 8 * g4) = w;
            }
        if constexpr (SPLIT) {  // the chunk's l and m of a real row, [B][NC][Nq][h]: what the combine weighs Oc with
            if (half == 0 && row_real(geo, qg * QMHA_GROUP + col)) {
                const size_t i = ((size_t)out_slice(geo, b) * Nq + (size_t)(qg * QMHA_GROUP + col - row_shift(geo))) * (size_t)(H * geo.G) + k;
                geo.pl[i] = l;
                geo.pm[i] = m_run;
            }
        }
    }
    }  // pass: the last stage's barrier has released both LDS buffers
