    // qmha_kv_append_int8.inc -- the body of qmha_kv_append_int8_kernel and qmha_kv_place_int8_kernel (qmha_prepass.hip).
    // In scope: D, `len` (the first cache row this wave's sequence writes), K, V, Ki, Vh, sK, sV, n, cap, H, d_model,
    // total_groups.
    __shared__ __attribute__((aligned(16))) char vtr[4][D * QMHA_VT_PITCH];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int item = blockIdx.x * 4 + wave;  // (bh, g)
    if (item >= total_groups) return;        // wave-uniform
    const int Gn = n / QMHA_GROUP, Gc = cap / QMHA_GROUP;
    const int bh = item / Gn, g = item % Gn;
    const int b = bh / H, k = bh % H;
    // quant_row_group / quant_v_group index source and destination by ONE row count: group g of n-row arrays,
    // element (bh n + 32 g) D of the rows, entry bh Gn + g of the scales and of the 64 D-byte V blocks.  They are
    // called with the chunk's n, which is right for the source; every destination pointer is moved ahead by what
    // the cache's index of the same group has more: group (bh Gc + len / 32 + g) - (bh Gn + g) = bh (Gc - Gn) +
    // len / 32 (>= 0, wave-uniform), so the functions -- and the pre-pass kernels built from them -- stay as they are.
    const size_t ahead = (size_t)bh * (Gc - Gn) + len / QMHA_GROUP;  // in groups
    if (blockIdx.y == 1)
        quant_v_group<D, 1>(V, Vh + ahead * (size_t)(32 * D), sV + ahead, vtr[wave], lane, b, k, g, bh, n, Gn, d_model);
    else
        quant_row_group<D>(K, Ki + ahead * (size_t)(QMHA_GROUP * D), sK + ahead, lane, b, k, g, bh, n, Gn, d_model);
