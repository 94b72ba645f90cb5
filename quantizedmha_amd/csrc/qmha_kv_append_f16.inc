    // qmha_kv_append_f16.inc -- the body of qmha_kv_append_f16_kernel and qmha_kv_place_f16_kernel (qmha_prepass.hip).
    // In scope: D, `len` (the first cache row this wave's sequence writes), K, V, Kh, Vt, n, cap, H, d_model, total_groups.
    constexpr int C4 = D / 4, RPI = 64 / C4, NI = 32 / RPI;
    __shared__ __attribute__((aligned(16))) char vtr[4][D * QMHA_VT_PITCH];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int item = blockIdx.x * 4 + wave;
    if (item >= total_groups) return;  // wave-uniform; the LDS tile is per wave, no workgroup barrier follows
    const int Gn = n / QMHA_GROUP, Gc = cap / QMHA_GROUP;
    const int bh = item / Gn, g = item % Gn;
    const int b = bh / H, k = bh % H;
    const int gd = len / QMHA_GROUP + g;
    v4f x[NI];
    if (blockIdx.y == 1) {  // V^T operand order: NI consecutive rows per lane (the vt_group_store map)
        const int rq = lane / C4, c4 = lane % C4;
        const float* base = V + ((size_t)b * n + (size_t)g * QMHA_GROUP) * d_model + (size_t)k * D + 4 * c4;
#pragma unroll
        for (int i = 0; i < NI; ++i)
            x[i] = __builtin_nontemporal_load(reinterpret_cast<const v4f*>(base + (size_t)(NI * rq + i) * d_model));
        vt_group_store<D, false>(vtr[wave], x, 1.0f, lane, reinterpret_cast<char*>(Vt + ((size_t)bh * Gc + gd) * (size_t)(32 * D)));
        return;
    }
    const int ri = lane / C4, ci = lane % C4;  // K: f16 rows
    const float* base = K + ((size_t)b * n + (size_t)g * QMHA_GROUP) * d_model + (size_t)k * D + 4 * ci;
#pragma unroll
    for (int i = 0; i < NI; ++i)
        x[i] = __builtin_nontemporal_load(reinterpret_cast<const v4f*>(base + (size_t)(i * RPI + ri) * d_model));
    _Float16* dst = Kh + ((size_t)bh * cap + (size_t)gd * QMHA_GROUP) * D + 4 * ci;
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        v4h hv;
#pragma unroll
        for (int c = 0; c < 4; ++c) hv[c] = (_Float16)x[i][c];  // RNE (= __float2half)
        *reinterpret_cast<v4h*>(dst + (size_t)(i * RPI + ri) * D) = hv;
    }
