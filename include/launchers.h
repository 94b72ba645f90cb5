/*
 * launchers.h -- C-ABI of the MI355X-native quantized multi-head attention library.
 *
 * Drop-in for the reference's include/launchers.h (MattJBorowski1991/QuantizedMHA).
 * Plain C types only: device pointers, sizes and an opaque stream handle (hipStream_t
 * passed as void*), so cgo/ctypes/JNI/N-API bindings need no HIP or torch headers.
 *
 * Libraries (built by tools/build.py):
 *   libqmha.so                 every entry point below; `solve` bound to fa_tc_int8_b
 *   libqmha_fa_tc_int8_b.so    `solve` bound to the INT8 path      (make KERNEL=fa_tc_int8_b)
 *   libqmha_fa_tc_v1a.so       `solve` bound to the FP16 MFMA path (make KERNEL=fa_tc_v1a)
 *   libqmha_fa.so              `solve` bound to the scalar path    (make KERNEL=fa)
 *   libqmha_fa_mfma.so         `solve` bound to fa's contract on the fp32 matrix cores
 *   libqmha_unfused.so         `solve` bound to the 3-kernel path  (make KERNEL=unfused)
 *   libqmha_fa_tc_int8_pt.so   `solve` bound to the per-tensor int8 mode (no reference kernel)
 * mirroring the reference's one-kernel-per-binary build (Makefile:39-53,
 * extensions/torch/setup.py:21-43).
 */
#ifndef QMHA_LAUNCHERS_H
#define QMHA_LAUNCHERS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Kernel variants (names as in the reference's mha_kernels/ and setup.py:114-124). */
typedef enum {
    QMHA_FA = 0,           /* mha_kernels/fa.cu         : fp32 scalar, no matrix cores   */
    QMHA_FA_TC_V1A = 1,    /* mha_kernels/fa_tc_v1a.cu  : fp16 MFMA, fp32 accumulation   */
    QMHA_FA_TC_INT8_B = 2, /* mha_kernels/fa_tc_int8_b.cu: int8 MFMA, per-32-row scales  */
    QMHA_UNFUSED = 3,      /* mha_kernels/unfused.cu    : QK^T, softmax, PV (3 kernels)   */
    QMHA_FA_MFMA = 4,      /* fa.cu's fp32 contract on v_mfma_f32_32x32x2_f32 (no reference
                              counterpart: the matrix-core sibling of the scalar `fa`)    */
    QMHA_FA_TC_INT8_PT = 5 /* per-tensor int8 mode (no reference counterpart: BASELINE.json's
                              "per-tensor Q/K/V quant", SURVEY 0.2's optional flag): one scale
                              per head slice of Q/K/V, static P scale 1/127, O accumulated on
                              the matrix core                                              */
} qmha_variant_t;

/* Status codes of the extended entry points. */
enum {
    QMHA_OK = 0,
    QMHA_ERR_INVALID = 1, /* shape/argument precondition failed (checked before launch) */
    QMHA_ERR_HIP = 2,     /* a HIP runtime call or kernel launch failed                  */
    QMHA_ERR_NOMEM = 3,   /* workspace allocation failed                                 */
    QMHA_ERR_NOSYS = 4    /* variant / head size not built into this library             */
};

/*
 * solve -- replaces the reference's `extern "C" void solve(...)` declared at
 * include/launchers.h:9-10 and defined per kernel (e.g. mha_kernels/fa_tc_int8_b.cu:600-609).
 *
 * Q, K, V, output: DEVICE pointers, fp32, contiguous [N, d_model] row-major; head k owns
 * columns [k*d, (k+1)*d), d = d_model / h.  output is fully overwritten.
 * Blocking: the result is complete on return (reference launchers.h:64).  Scratch is
 * owned by the library.  Preconditions (the reference asserts N % 32 on the device,
 * fa_tc_int8_b.cu:422-423): N % 32 == 0, d_model == h*d, d % 32 == 0 (config.h:32) and d <= 256
 * (fa_tc_int8_pt, the per-tensor mode with no reference counterpart: d in {32, 64, 128}).  The
 * reference's d is a compile-time constant (config.h:28); here it is a runtime value.
 * On a violated precondition or HIP error `solve` prints one line to stderr and returns
 * (the reference returns void and ignores errors).
 */
void solve(const float *Q, const float *K, const float *V, float *output, int N, int d_model, int h);

/*
 * qmha_solve_ex -- batched, asynchronous, status-returning form of `solve`.
 * Q/K/V/O are [B, N, d_model] fp32 device tensors (batch outermost; B calls of the
 * reference `solve`).  Work is enqueued on `stream` (hipStream_t, NULL = default stream)
 * and the call returns without synchronising.  A library-owned workspace is cached per
 * (device, stream); see qmha_solve_ws for caller-owned scratch (graph capture).
 */
int qmha_solve_ex(const float *Q, const float *K, const float *V, float *O, int B, int N, int d_model, int h,
                  int variant, void *stream);

/* Bytes of scratch qmha_solve_ws needs for this problem (0 for variants without). */
size_t qmha_workspace_size(int B, int N, int d_model, int h, int variant);

/* As qmha_solve_ex with caller-owned device scratch of >= qmha_workspace_size bytes
 * (256-byte aligned).  Makes no allocation and no synchronisation: capturable in a hipGraph. */
int qmha_solve_ws(const float *Q, const float *K, const float *V, float *O, int B, int N, int d_model, int h,
                  int variant, void *workspace, size_t workspace_bytes, void *stream);

/* Option flags of qmha_solve_opts. */
enum {
    QMHA_FLAG_CAUSAL = 1 /* query row r attends keys j <= r of its own sequence (Nq = Nk = N);
                            Nq != Nk: qmha_solve_rect, bottom-right aligned, j <= r + (Nk - Nq) */
};

/*
 * qmha_solve_opts -- qmha_solve_ex / qmha_solve_ws with option flags.  workspace == NULL: the
 * library-owned, leased workspace of qmha_solve_ex (workspace_bytes is ignored).  Otherwise the
 * qmha_solve_ws rules: caller-owned scratch of >= qmha_workspace_size bytes (the same size with or
 * without flags), no allocation, no synchronisation, capturable in a hipGraph.  flags == 0 enqueues
 * exactly what qmha_solve_ex / qmha_solve_ws enqueue.  Unknown flag bits: QMHA_ERR_INVALID.
 * QMHA_FLAG_CAUSAL is built for fa_tc_int8_b at d = 32, 64, 128 and fa_tc_v1a at d = 64, 128; every
 * other variant or head size returns QMHA_ERR_NOSYS (qmha_last_error names the variant and d) before
 * anything is launched, leaving O untouched.
 */
int qmha_solve_opts(const float *Q, const float *K, const float *V, float *O, int B, int N, int d_model, int h,
                    int variant, unsigned flags, void *workspace, size_t workspace_bytes, void *stream);

/*
 * qmha_solve_rect -- qmha_solve_opts with separate query and key lengths: cross-attention and chunked
 * prefill.  Q and O are [B, Nq, d_model], K and V are [B, Nk, d_model] (fp32, contiguous, batch outermost).
 * Stream, status, leased-slot and caller-workspace rules are qmha_solve_opts': workspace == NULL uses the
 * library's slot; otherwise the caller supplies >= qmha_workspace_size(B, Nk, d_model, h, variant) bytes (the
 * scratch depends on the key length only) and the call makes no allocation and no synchronisation.
 * flags == 0: every query row attends all Nk keys (any Nq, Nk, also Nq > Nk).  QMHA_FLAG_CAUSAL: bottom-right
 * aligned, query row r attends keys j <= r + (Nk - Nq) -- the Nq queries are the last Nq positions of a
 * sequence of Nk; needs Nk >= Nq (QMHA_ERR_INVALID otherwise).  Nq % 32 == 0 and Nk % 32 == 0; the other
 * preconditions are qmha_solve_ex's, per tensor.  Unknown flag bits: QMHA_ERR_INVALID.
 * Nq == Nk enqueues exactly what qmha_solve_opts enqueues, for every variant.  Nq != Nk is built for
 * fa_tc_int8_b at d = 32, 64, 128 and fa_tc_v1a at d = 64, 128, with or without QMHA_FLAG_CAUSAL; every other
 * variant or head size returns QMHA_ERR_NOSYS (qmha_last_error names the variant and d) before anything is
 * launched, leaving O untouched.  Every call runs the K/V pre-pass over all Nk rows (qmha_kv_cache_* below keeps
 * the pre-passed rows of earlier calls instead).
 */
int qmha_solve_rect(const float *Q, const float *K, const float *V, float *O, int B, int Nq, int Nk, int d_model,
                    int h, int variant, unsigned flags, void *workspace, size_t workspace_bytes, void *stream);

/*
 * qmha_solve_gqa -- qmha_solve_rect for grouped-query attention (GQA; h_kv = 1: MQA): the h query heads share
 * h_kv key/value heads, query head k reading K/V head k / (h / h_kv).  Q and O are [B, Nq, d_model]; K and V are
 * [B, Nk, h_kv * (d_model / h)] (fp32, contiguous, batch outermost).  1 <= h_kv <= h and h % h_kv == 0, otherwise
 * QMHA_ERR_INVALID; every other rule is qmha_solve_rect's (Nq % 32 == 0, Nk % 32 == 0, QMHA_FLAG_CAUSAL bottom-right
 * aligned and Nk >= Nq, unknown flag bits QMHA_ERR_INVALID, every check before any HIP call).
 * There is no size function of its own: K, V and the scratch are those of a call with h_kv heads, so a caller
 * workspace holds >= qmha_workspace_size(B, Nk, h_kv * (d_model / h), h_kv, variant) bytes.
 * h_kv == h enqueues exactly what qmha_solve_rect enqueues, for every variant and shape.  h_kv < h is built for
 * fa_tc_int8_b at d = 32, 64, 128 and fa_tc_v1a at d = 64, 128 (qmha_solve_rect's Nq != Nk set) and runs the
 * grouped kernels for every Nq and Nk, square and unmasked calls included; every other variant or head size
 * returns QMHA_ERR_NOSYS (qmha_last_error names the variant, d and "grouped-query") before anything is launched,
 * leaving O untouched.  The K/V pre-pass runs once per K/V head, and query head k's result is bit-identical to
 * qmha_solve_rect on K and V expanded to h heads whenever that call takes its rectangular kernel.
 */
int qmha_solve_gqa(const float *Q, const float *K, const float *V, float *O, int B, int Nq, int Nk, int d_model, int h,
                   int h_kv, int variant, unsigned flags, void *workspace, size_t workspace_bytes, void *stream);

/*
 * Persistent K/V cache -- chunked prefill and decode without re-running the K/V pre-pass over rows that were
 * quantised (int8) or converted (fp16) by an earlier call.  A cache is an opaque host object over CALLER-OWNED device
 * memory: qmha_kv_cache_bytes(B, cap, ...) bytes (exactly qmha_workspace_size at N = cap; the layout is that
 * workspace's), 256-byte aligned, holding up to `cap` rows of K and V per sequence, of which the first `len` are valid.
 * The library never allocates, frees or synchronises for a cache; destroy releases the host object only.
 *
 *   create    cap % 32 == 0, cap >= 32, the other shape rules of qmha_solve_ex at N = cap; len = 0.  Built for
 *             fa_tc_int8_b at d = 32, 64, 128 and fa_tc_v1a at d = 64, 128 (qmha_solve_rect's Nq != Nk set); any other
 *             variant or head size: QMHA_ERR_NOSYS, qmha_last_error names the variant and d.
 *   append    K, V: [B, n, d_model] fp32 device tensors, contiguous; n % 32 == 0, n >= 32, len + n <= cap (otherwise
 *             QMHA_ERR_INVALID and len is unchanged).  Enqueues the pre-pass of the n new rows on `stream`, writing
 *             rows [len, len + n) of the cache with the bytes the pre-pass of a whole call writes for them (32-row
 *             quantisation groups are independent); len advances by n only when the launch succeeded.
 *   attend    Q, O: [B, Nq, d_model], Nq % 32 == 0.  QMHA_FLAG_CAUSAL: bottom-right aligned over the valid rows,
 *             query row r attends cache rows j <= r + (len - Nq); needs Nq <= len.  Rows at and beyond len are never
 *             read, whatever they hold.  flags == 0: every query row attends all cap rows, which needs len == cap (a
 *             cross-attention memory built once at its size); len < cap without the mask is QMHA_ERR_INVALID.  Unknown
 *             flag bits: QMHA_ERR_INVALID.  The result is bit-identical to qmha_solve_rect(Q, K[:, :len], V[:, :len],
 *             Nq, len, flags) whenever that call takes its rectangular kernel (Nq != len, or no mask).
 *   truncate  drops rows from the end: len % 32 == 0, 0 <= len <= the current length.  Host only; nothing is enqueued.
 *   len       the valid rows; 0 after create.
 *
 * Every check runs before any HIP call.  append and attend make no allocation and no synchronisation, so they can
 * be captured in a hipGraph; the capture bakes in the cache's length at the time of the call (a replay appends to,
 * and attends over, the same rows again).
 * Threading: each cache has a mutex of its own, held across an enqueue; no leased (device, stream) slot is taken.
 * Different caches are independent and may be used from different threads and streams at once.  The CALLER orders
 * the operations on one cache: by issuing them on one stream, or with its own events -- an attend must follow the
 * appends it reads, and an append into rows freed by truncate must follow the attends that still read them.
 * With qmha_profile_enable(1), every append records one pre-pass event pair and every attend one main-kernel pair,
 * each a record of its own (qmha_profile_collect counts one call for each).
 *
 * qmha_kv_cache_create_gqa: a cache of h_kv key/value heads shared by h query heads (the rules of qmha_solve_gqa;
 * h_kv == h is qmha_kv_cache_create).  The memory is qmha_workspace_size(B, cap, h_kv * (d_model / h), h_kv, variant)
 * bytes -- qmha_kv_cache_bytes at h_kv heads, 1 / (h / h_kv) of the multi-head cache --, append takes K, V of
 * [B, n, h_kv * (d_model / h)], attend takes Q, O of [B, Nq, d_model] as before and runs the grouped kernels;
 * truncate and len are unchanged.  h_kv < h with a variant or head size outside qmha_solve_gqa's set: QMHA_ERR_NOSYS.
 */
typedef struct qmha_kv_cache qmha_kv_cache_t;
size_t qmha_kv_cache_bytes(int B, int cap, int d_model, int h, int variant);
int qmha_kv_cache_create(qmha_kv_cache_t **out, void *mem, size_t bytes, int B, int cap, int d_model, int h,
                         int variant);
int qmha_kv_cache_create_gqa(qmha_kv_cache_t **out, void *mem, size_t bytes, int B, int cap, int d_model, int h,
                             int h_kv, int variant);
void qmha_kv_cache_destroy(qmha_kv_cache_t *c);
int qmha_kv_cache_len(const qmha_kv_cache_t *c);
int qmha_kv_cache_truncate(qmha_kv_cache_t *c, int len);
int qmha_kv_cache_append(qmha_kv_cache_t *c, const float *K, const float *V, int n, void *stream);
int qmha_attend_cached(qmha_kv_cache_t *c, const float *Q, float *O, int Nq, unsigned flags, void *stream);

/*
 * Per-sequence lengths, read on the device -- a batch whose sequences differ in length in one cache, and a decode step
 * that is captured once and replayed while the lengths advance in device memory.  pos and lens are DEVICE int32[B]
 * arrays that the kernels read when they run; the host never reads them, so nothing is baked into a capture but the
 * two pointers.  Both calls address the rows append / attend address (they may be mixed with them on one cache) and
 * neither reads or changes the cache's host `len`: the caller owns the lengths.  Multi-head and grouped caches alike.
 *
 *   append_at      K, V: [B, n, h_kv * d] as for append; n % 32 == 0, 32 <= n <= cap, checked on the host.  Sequence b's n
 *                  rows go to cache rows [pos[b], pos[b] + n), with the bytes append writes for them at len == pos[b];
 *                  nothing else is written.  On the device, pos[b] is valid when pos[b] >= 0, pos[b] % 32 == 0 and
 *                  pos[b] + n <= cap; a sequence with an invalid pos[b] writes nothing at all (a slot left out of a step).
 *   attend_varlen  Q, O: [B, Nq, d_model], Nq % 32 == 0; flags as for attend; QMHA_FLAG_CAUSAL needs Nq <= cap; checked
 *                  on the host.  On the device, L = lens[b] is valid when L % 32 == 0, L <= cap and L >= Nq (causal) or
 *                  L >= 32 (flags == 0).  A valid sequence computes what attend computes at len == L, bit for bit: causal,
 *                  row r attends rows j <= r + (L - Nq); flags == 0, every row attends rows [0, L) -- also at L < cap,
 *                  which attend cannot do.  Rows at and beyond L are never read.  An invalid sequence (L == 0: an empty
 *                  slot) has its Nq rows of O written as zeros and none of its K/V read.
 *
 * Null pos / lens: QMHA_ERR_INVALID.  Every host check runs before any HIP call; no allocation, no synchronisation;
 * the cache's mutex is held across the enqueue; qmha_profile records are those of append / attend.
 */
int qmha_kv_cache_append_at(qmha_kv_cache_t *c, const float *K, const float *V, int n, const int32_t *pos, void *stream);
int qmha_attend_cached_varlen(qmha_kv_cache_t *c, const float *Q, float *O, int Nq, const int32_t *lens, unsigned flags,
                              void *stream);

/*
 * Token-granular lengths -- append and attend at any length: a prompt of 1000 tokens, a decode step of one.  Device
 * lengths only, as above: pos and lens are DEVICE int32[B] arrays read by the kernels, the host `len` is neither read
 * nor changed, multi-head and grouped caches alike.  Absolute row positions of a sequence keep their 32-row groups, and
 * a ragged call is DEFINED as the call above on zero-padded operands, which it matches bit for bit:
 *
 *   keys / values  a cache that holds L rows of a sequence holds the bytes append_at writes for those rows zero-padded
 *                  to L' = ceil32(L).  For int8 the open (last, partial) group's scale comes from the rows present --
 *                  zero rows do not move an absmax -- and the group is quantised again from its raw rows every time
 *                  rows are added; it is final once it is full.
 *   queries        Nq rows attend a sequence of L rows, causal and bottom-right aligned: row r sees keys j <= r + L - Nq.
 *                  With s = (L - Nq) mod 32 and Nq' = ceil32(s + Nq) the result is rows [s, s + Nq) of attend_varlen's
 *                  causal call on a zero [Nq', d_model] block that holds Q at rows [s, s + Nq), against L' rows (L' - Nq'
 *                  is a multiple of 32, and the diagonal mask hides exactly the zero key rows >= L from every real row).
 *                  A single-token decode step: s = (L - 1) mod 32, Nq' = 32.  int8: the zero query rows have p = 1 on the
 *                  keys they see and enter the P tile's absmax, so a tile shared with pad rows is quantised with
 *                  sP = 1/127, the per-tensor mode's static scale (DESIGN.md 17 has the measured accuracy).
 *
 *   tail_bytes     the bytes of caller-owned device memory for the raw fp32 rows of each sequence's open group: int8, K and
 *                  V of 32 rows x h_kv * d per sequence; fp16, 0 (a row converts on its own).
 *   attach_tail    attaches that memory (256-byte aligned, >= tail_bytes, otherwise QMHA_ERR_INVALID) to the cache.  A
 *                  buffer of its own: the cache memory and qmha_kv_cache_bytes stay as they are.  The library never
 *                  allocates or frees it.  fp16: nothing to attach, QMHA_OK.
 *   append_tokens  K, V: [B, n, h_kv * d], any 1 <= n <= cap (host check).  On the device, pos[b] is valid when
 *                  pos[b] >= 0 and pos[b] + n <= cap: the 32-row groups that rows [pos[b], pos[b] + n) touch get the bytes
 *                  of the contract above, no other group is written, and the tail is updated.  An invalid pos[b]: nothing
 *                  is written, the tail included.  An int8 cache without a tail: QMHA_ERR_INVALID.
 *                  An append that starts inside a group (pos[b] % 32 != 0) RELIES on the tail holding that group's earlier
 *                  rows (int8), and on the group's rows behind them being zero (fp16), from the append_tokens calls that
 *                  wrote them: build a partial group with append_tokens from its first row on.  append / append_at at a
 *                  multiple of 32 start a fresh group and need no tail; so does append_tokens there.
 *   attend_tokens  Q, O: [B, Nq, d_model], any 1 <= Nq <= cap; flags must be QMHA_FLAG_CAUSAL (the kernels have no mask but
 *                  the diagonal: unmasked ragged attention is not built), anything else QMHA_ERR_INVALID; host checks.
 *                  On the device, L = lens[b] is valid when Nq <= L <= cap: the contract above.  Rows at and beyond
 *                  ceil32(L) are never read; Q and O are touched at their Nq rows only.  An invalid L: the sequence's Nq
 *                  rows of O are positive zeros and none of its K/V is read.
 *
 * Null pos / lens: QMHA_ERR_INVALID.  Every host check runs before any HIP call; no allocation, no synchronisation (both
 * calls can be captured in a hipGraph); the cache's mutex is held across the enqueue; qmha_profile records are those of
 * append / attend.
 */
size_t qmha_kv_cache_tail_bytes(const qmha_kv_cache_t *c);
int qmha_kv_cache_attach_tail(qmha_kv_cache_t *c, void *mem, size_t bytes);
int qmha_kv_cache_append_tokens(qmha_kv_cache_t *c, const float *K, const float *V, int n, const int32_t *pos, void *stream);
int qmha_attend_cached_tokens(qmha_kv_cache_t *c, const float *Q, float *O, int Nq, const int32_t *lens, unsigned flags,
                              void *stream);

/*
 * Paged caches -- a pool of pages and a block table, for a server whose sequences come, grow and go: memory follows the
 * rows that exist, a finished sequence's pages go to another slot, and sequences with a common prompt share its pages.
 * A paged call is DEFINED as the token-granular call above with the row address looked up through the table, and
 * matches it bit for bit.  Multi-head and grouped caches alike; causal only.
 *
 *   page           page_rows rows of all h_kv K/V heads of one sequence; page_rows % 64 == 0, page_rows >= 64 (a stage of
 *                  the kernels is two 32-row key tiles, so it never straddles pages).
 *   pool           num_pages pages: the variant's workspace carve with B := num_pages, N := page_rows, H := h_kv.  Page p,
 *                  K/V head kvh is head slice p * h_kv + kvh of every array.  paged_bytes(num_pages, page_rows, d_model, h,
 *                  h_kv, variant) == qmha_workspace_size(num_pages, page_rows, h_kv * d, h_kv, variant): nothing new is
 *                  laid out, and 32-row quantisation groups are independent, so a page holds the same bytes wherever it is.
 *   table          a DEVICE int32 [B][max_pages] array, row-major, caller-owned, passed with every call and read by the
 *                  kernels when they run, like pos and lens: the host never reads it, so a captured step follows a table
 *                  that the caller advances in device memory.  Row r of sequence b lives in page table[b][r / page_rows]
 *                  at row r % page_rows; a sequence's logical capacity is cap = max_pages * page_rows.  The caller owns
 *                  the allocation policy: the library keeps no free list.
 *   create_paged   the handle of the calls above, marked paged; B is the number of sequence slots.  page_rows % 64 != 0,
 *                  num_pages < 1, max_pages < 1, memory not 256-byte aligned or below paged_bytes: QMHA_ERR_INVALID; the
 *                  head rules and QMHA_ERR_NOSYS of qmha_kv_cache_create_gqa.  qmha_kv_cache_len of a paged cache is 0.
 *   tail           qmha_kv_cache_tail_bytes / _attach_tail as above.  The tail belongs to the B sequence slots, not to
 *                  pages: [2][B][32][h_kv * d].
 *   append_paged   K, V: [B, n, h_kv * d], any 1 <= n <= cap (host check).  On the device, sequence b is valid when
 *                  pos[b] >= 0, pos[b] + n <= cap and every table entry that rows [pos[b], pos[b] + n) use lies in
 *                  [0, num_pages).  It leaves, in every page it touches, the bytes append_tokens leaves in those rows of a
 *                  contiguous cache; other pages, other groups and the rows at and beyond ceil32(pos[b] + n) are neither
 *                  read nor written.  An invalid sequence writes nothing, the tail included.  The rule on partial groups
 *                  is append_tokens': build one with append_paged from its first row on.
 *   attend_paged   Q, O: [B, Nq, d_model], any 1 <= Nq <= cap; flags must be QMHA_FLAG_CAUSAL (host checks).  On the device,
 *                  sequence b is valid when Nq <= lens[b] <= cap and every table entry of pages 0 .. ceil(lens[b] /
 *                  page_rows) - 1 lies in [0, num_pages): O holds the bits of attend_tokens on the contiguous cache.  An
 *                  invalid sequence: its Nq rows of O are positive zeros and none of its K/V is read.  Entries behind the
 *                  pages a call uses are not looked at (a caller may keep -1 there), and no table content is ever turned
 *                  into an address outside the pool.
 *   sharing        two sequences may name the same page in an attend: prefix sharing, read-only.  Two sequences WRITING one
 *                  page in one append_paged is the caller's error: the result in that page is unspecified and nothing else
 *                  is affected.  Leave a sequence out of an append with pos[b] = -1.
 *
 * The contiguous entry points (append, attend, append_at, attend_varlen, append_tokens, attend_tokens, truncate) on a
 * paged cache return QMHA_ERR_INVALID, and so do the paged entry points on a contiguous cache.  Null pos / lens / table:
 * QMHA_ERR_INVALID.  Every host check runs before any HIP call; no allocation, no synchronisation (both calls can be
 * captured in a hipGraph); the cache's mutex is held across the enqueue; qmha_profile records are those of append / attend.
 */
size_t qmha_kv_cache_paged_bytes(int num_pages, int page_rows, int d_model, int h, int h_kv, int variant);
int qmha_kv_cache_create_paged(qmha_kv_cache_t **out, void *mem, size_t bytes, int B, int num_pages, int page_rows,
                               int max_pages, int d_model, int h, int h_kv, int variant);
int qmha_kv_cache_append_paged(qmha_kv_cache_t *c, const float *K, const float *V, int n, const int32_t *pos,
                               const int32_t *table, void *stream);
int qmha_attend_cached_paged(qmha_kv_cache_t *c, const float *Q, float *O, int Nq, const int32_t *lens, const int32_t *table,
                             unsigned flags, void *stream);

/*
 * Split-KV -- attend_tokens / attend_paged with the key sweep cut into chunks, for a decode step (small Nq, long
 * sequences), where the unsplit call runs one wave per head along the whole sequence.  Everything the two calls above
 * state holds: device lens and table, any 1 <= Nq <= cap, causal only, the validity rules, multi-head and grouped caches.
 * The result is a deterministic function of its own, inside the same accuracy contract; it is not the
 * unsplit call's bits.
 *
 *   chunk_rows     key rows per chunk: a multiple of 64 with 64 <= chunk_rows <= cap, so C = chunk_rows / 32 tiles are a
 *                  whole number of two-tile stages (and never cut a page's stage).  NC = ceil(cap / chunk_rows) chunks.
 *   partial        first launch.  For sequence b, 32-row query group qg (the padded groups of the token-granular contract)
 *                  and every chunk c with c * C <= last(qg), one wave runs the tiles c * C ... min(c * C + C - 1, last(qg))
 *                  of the unsplit kernel from the zero state and ends with its epilogue: it stores, for real rows only,
 *                  Oc = O / l (0 where l is at or below the variant's threshold), the row sum l and the running maximum m
 *                  (log2 units) of those tiles alone -- bit for bit what the unsplit kernel computes over those key tiles.
 *                  Chunks a group does not reach are not written.
 *   combine        second launch, same stream; the only writer of O.  Per real row and head, over the chunks
 *                  c = 0 ... last(qg) / C in ascending order, in fp32: M = max m_c, a_c = l_c * exp2(m_c - M),
 *                  Ltot = sum a_c, O = Ltot > thr ? (sum a_c * Oc_c) / Ltot : 0 (thr: 1e-20 int8, 1e-10 fp16).  An invalid
 *                  sequence (its lens[b], or a used table entry outside the pool): Nq rows of positive zeros, no scratch read.
 *   scratch        caller-owned device memory, 256-byte aligned, qmha_attend_split_bytes(c, Nq, chunk_rows) bytes (0 on
 *                  invalid arguments), never allocated or synchronised by the call.  Three fp32 arrays, each starting on
 *                  a multiple of 256 bytes, in this order:
 *                      Oc [B][NC][Nq][h * d]      m [B][NC][Nq][h]      l [B][NC][Nq][h]
 *                  Entries of chunks a row does not reach keep what they held.  Two calls in flight on different streams
 *                  need different scratch.
 *
 * Host checks, all before any HIP call, QMHA_ERR_INVALID: null cache / Q / O / lens / table / scratch, Nq outside
 * [1, cap], flags other than QMHA_FLAG_CAUSAL, chunk_rows no multiple of 64, below 64 or above cap, scratch misaligned or
 * below qmha_attend_split_bytes, the contiguous entry point on a paged cache and the reverse.  No allocation, no
 * synchronisation, no atomics, no waiting between workgroups (both launches can be captured in a hipGraph); one
 * qmha_profile main pair covers both launches.
 */
size_t qmha_attend_split_bytes(const qmha_kv_cache_t *c, int Nq, int chunk_rows);
int qmha_attend_cached_tokens_split(qmha_kv_cache_t *c, const float *Q, float *O, int Nq, const int32_t *lens,
                                    int chunk_rows, void *scratch, size_t scratch_bytes, unsigned flags, void *stream);
int qmha_attend_cached_paged_split(qmha_kv_cache_t *c, const float *Q, float *O, int Nq, const int32_t *lens,
                                   const int32_t *table, int chunk_rows, void *scratch, size_t scratch_bytes, unsigned flags,
                                   void *stream);

/*
 * Packed batches -- a query count and an append count per sequence in one call, for a continuous-batching step that
 * mixes chunked prefill and decode.  The operands have no batch axis, in the cu_seqlens convention of varlen attention:
 *
 *   Q, O           [total, d_model]          K, V  [total, h_kv * d]
 *   cu             a DEVICE int32 [B + 1] array, caller-owned, read by the kernels when they run, like pos, lens and
 *                  table: sequence b owns the rows [cu[b], cu[b + 1]) of the packed operands, n_b = cu[b + 1] - cu[b] of
 *                  them.  The host never reads it, so a captured step follows a mix the caller changes in device memory.
 *                  One cu array may serve the append and the attend of a step.  A monotone cu is the caller's side of
 *                  the contract: ranges of different sequences that overlap stay in bounds, their content is unspecified.
 *   total          the rows of the packed operands (host); rows outside every range are neither read nor written.
 *   max_n, max_nq  an upper bound (host) of the counts, 1 <= bound <= min(total, cap): it sizes the grid, as n and Nq do
 *                  for the calls above.
 *
 * The contract is the calls' above, per sequence and bit for bit.  Multi-head, grouped and paged caches; causal only.
 *
 *   append_packed, append_paged_packed
 *                  a sequence with 1 <= n_b <= max_n rows, pos[b] >= 0 and pos[b] + n_b <= cap (paged: and every table
 *                  entry the rows touch in [0, num_pages)): the cache and the tail hold afterwards what append_tokens
 *                  (append_paged) with n = n_b writes for it; no other group is written.  n_b == 0: the sequence sits
 *                  out, pos[b] is not looked at.  Any other sequence writes nothing, the tail included.
 *   attend_packed, attend_paged_packed
 *                  a sequence with 1 <= nq_b <= max_nq rows and nq_b <= lens[b] <= cap (paged: and every used table entry
 *                  in the pool): its rows of O are the rows attend_tokens (attend_paged) writes for a sequence of that
 *                  Nq and lens[b] over the same cache bytes.  nq_b == 0: the sequence sits out, lens[b] is not looked at.
 *                  Any other sequence whose range is in bounds: its rows of O are positive zeros, none of its K/V is read.
 *   range          in bounds when 0 <= cu[b] <= cu[b + 1] <= total.  A range that is not never becomes an address: nothing
 *                  of that sequence is read or written.
 *
 * Host checks, all before any HIP call, QMHA_ERR_INVALID: null cache / tensor / cu / pos / lens / table, total < 1,
 * max_n or max_nq outside [1, min(total, cap)], flags other than QMHA_FLAG_CAUSAL, an int8 cache without its tail, the
 * contiguous entry point on a paged cache and the reverse.  No allocation, no synchronisation (the calls can be captured
 * in a hipGraph); the cache's mutex is held across the enqueue; qmha_profile records are those of append / attend.
 */
int qmha_kv_cache_append_packed(qmha_kv_cache_t *c, const float *K, const float *V, int total, int max_n, const int32_t *cu,
                                const int32_t *pos, void *stream);
int qmha_kv_cache_append_paged_packed(qmha_kv_cache_t *c, const float *K, const float *V, int total, int max_n,
                                      const int32_t *cu, const int32_t *pos, const int32_t *table, void *stream);
int qmha_attend_cached_packed(qmha_kv_cache_t *c, const float *Q, float *O, int total, int max_nq, const int32_t *cu,
                              const int32_t *lens, unsigned flags, void *stream);
int qmha_attend_cached_paged_packed(qmha_kv_cache_t *c, const float *Q, float *O, int total, int max_nq, const int32_t *cu,
                                    const int32_t *lens, const int32_t *table, unsigned flags, void *stream);

/*
 * Sliding-window attention -- qmha_attend_cached_tokens / qmha_attend_cached_paged in which a query row sees only the
 * last `window` keys of those the causal mask leaves it (Mistral-style layers, local/global alternation).  Everything
 * is the unwindowed call's -- Q, O [B, Nq, d_model], any 1 <= Nq <= cap; the DEVICE arrays lens and table; multi-head,
 * grouped and paged caches of every built (variant, d); flags must be QMHA_FLAG_CAUSAL -- except:
 *
 *   the mask       with L = lens[b], real row i of the Nq rows attends the cache rows j with
 *                  i + L - Nq - window < j <= i + L - Nq: exactly min(window, i + L - Nq + 1) keys.
 *   window         a host int, a multiple of 32, >= 32, with no upper limit (absolute row positions keep their 32-row
 *                  groups, so the window's left edge falls on a key tile's diagonal).  A window that reaches the start of
 *                  every sequence (window >= cap) gives the unwindowed call's O bit for bit.
 *   the sweep      query group qg (the 32-row group of absolute positions) sweeps the key tiles first(qg) ... diag(qg),
 *                  first(qg) = max(0, diag(qg) - window / 32), from the zero state; tiles before first(qg) are neither
 *                  staged for that group's sake nor computed, so a decode step costs window / 32 + 1 tiles whatever L is.
 *                  A ragged call is, as for attend_tokens, the call on the zero-padded block against ceil32(L) rows.
 *   paged          only the table columns whose pages hold rows [64 * (first(0) / 2), L) of the sequence are used: the
 *                  window, widened to the two-tile stage that holds its first tile.  Columns behind them are not loaded --
 *                  they may hold anything, -1 for instance, and their pages may have been given to another sequence.  A
 *                  used entry outside [0, num_pages): the sequence's rows of O are positive zeros, none of its K/V is read.
 *
 * Validity on the device is the unwindowed call's: Nq <= lens[b] <= cap, any other length gives positive zeros and
 * nothing read.  Host checks, all before any HIP call, QMHA_ERR_INVALID: those of the unwindowed call in their order,
 * then window < 32 or window % 32 != 0.  No allocation, no synchronisation (the calls can be captured in a hipGraph);
 * the cache's mutex is held across the enqueue; the qmha_profile record is attend's.
 */
int qmha_attend_cached_tokens_window(qmha_kv_cache_t *c, const float *Q, float *O, int Nq, const int32_t *lens, int window,
                                     unsigned flags, void *stream);
int qmha_attend_cached_paged_window(qmha_kv_cache_t *c, const float *Q, float *O, int Nq, const int32_t *lens,
                                    const int32_t *table, int window, unsigned flags, void *stream);

/* Blocking convenience used by the per-variant `solve` shims and the JAX raw-pointer
 * binding (extensions/jax/jax_ext.cpp:12-28): batch 1, synchronises the device stream. */
int qmha_solve_variant(const float *Q, const float *K, const float *V, float *O, int N, int d_model, int h,
                       int variant);

/*
 * qmha_quantize_int8 -- the INT8 path's pre-pass as a standalone op:
 * per 32-row group of every head, scale = max(absmax/127, 1e-8) and
 * x_i8 = clamp(rint(x / scale), -128, 127) (fa_tc_int8_b.cu:33-152, fp32_to_int8sram).
 * X: [B, N, d_model] fp32 device.  Xi: [B][h][N][d] int8 device.  scales: [B][h][N/32].
 * layout 0 = row-major rows (Q, K operand); layout 1 = V^T MFMA operand order
 * ([B][h][N/32][d][32], kv slots permuted as documented in DESIGN.md); layout 2 = row-major rows
 * with ONE scale per head slice (the fa_tc_int8_pt per-tensor mode; scales: [B][h]).
 */
int qmha_quantize_int8(const float *X, int B, int N, int d_model, int h, int8_t *Xi, float *scales, int layout,
                       void *stream);

/*
 * qmha_debug_qk_int32 -- test hook for the bit-exact KAT: quantises Q and K exactly as the
 * INT8 path does and writes S = Q_i8 K_i8^T (int32) of head `head` (batch 0) computed by
 * the same v_mfma_i32_32x32x32_i8 operand path into S[N][N] (device).  Blocking.
 */
int qmha_debug_qk_int32(const float *Q, const float *K, int N, int d_model, int h, int head, int32_t *S);

/*
 * Test hook (the bit-exact int32 Q@K^T check, reference fa_tc_int8_b.cu:484,496,514):
 * runs the PRODUCTION int8 schedule (same kernel template and flags as qmha_solve_ex, plus the
 * FL_DUMP stores) and writes what that kernel itself computed: O as qmha_solve_ex would, the
 * int32 S = Qi Ki^T of every (sequence, head) as its MFMAs produced it (accumulator bias
 * removed) into S[B*h][N][N], its in-register int8 Q operand into Qi[B*h][N][d] and the Q
 * group scales into sQ[B*h][N/32].  N >= 64.  Device pointers; blocking.
 */
int qmha_debug_fa_int8_dump(const float *Q, const float *K, const float *V, float *O, int B, int N, int d_model,
                            int h, int32_t *S, int8_t *Qi, float *sQ);

/* As qmha_debug_fa_int8_dump for the per-tensor mode (QMHA_FA_TC_INT8_PT): its production schedule
 * plus the stores; Qi is quantised with the head slice's scale, and sQ[B*h][N/32] holds that one
 * scale in every group's entry.  N >= 32.  Device pointers; blocking. */
int qmha_debug_fa_int8_pt_dump(const float *Q, const float *K, const float *V, float *O, int B, int N, int d_model,
                               int h, int32_t *S, int8_t *Qi, float *sQ);

/*
 * Test hook: the P stage of the per-block int8 path (QMHA_FA_TC_INT8_B), tile by tile.  Takes Nq, Nk and flags
 * as qmha_solve_rect and launches the dumping twin of whichever main kernel that call would launch (the
 * pipelined kernel, the one-tile kernel -- N = 32 included --, or the causal / rectangular kernel), which
 * writes O as in production and, for every tile a wave computes (Gq = Nq/32, Gk = Nk/32, key tile t):
 *   S  [B*h][Nq][Nk]    int32  Qi Ki^T as the MFMAs produced it, before the causal mask
 *   Qi [B*h][Nq][d]     int8   the in-register Q operand;  sQ [B*h][Gq] its group scales
 *   m  [B*h][Nq][Gk]    fp32   the row's running max after tile t (log2 units)
 *   sP [B*h][Gq][Gk]    fp32   the tile's P scale
 *   Pi [B*h][Nq][Nk]    int8   the quantised P entry, read back from the packed f16 operand of the P@V MFMA
 *   T  [B*h][Gk][Nq][d] int32  the tile's P@V accumulator (INT32_MIN: the accumulator was not an integer)
 *   l  [B*h][Nq]        fp32   the row sum the epilogue divides by
 * Entries of tiles a wave does not visit (past the diagonal of a causal call) are left untouched.
 * Device pointers; runs on the null stream; blocking.
 */
int qmha_debug_fa_int8_pstage(const float *Q, const float *K, const float *V, float *O, int B, int Nq, int Nk,
                              int d_model, int h, unsigned flags, int32_t *S, int8_t *Qi, float *sQ, float *m,
                              float *sP, int8_t *Pi, int32_t *T, float *l);

/* Test hook: bound, in ticks of the 100 MHz real-time clock, of the per-tensor pre-pass's wait for the
 * other parts of a head slice (default 200000 = 2 ms; 0 makes every part take its fallback, reducing
 * the whole slice itself; negative makes every call take the two-pass form that slices of more parts
 * than one XCD holds at once always take -- the same scales, bit-identical output).  Returns the
 * previous bound. */
int64_t qmha_debug_set_pt_wait(int64_t ticks);

/* Variant name ("fa", "fa_tc_v1a", "fa_tc_int8_b", "unfused", "fa_mfma", "fa_tc_int8_pt") -> id, or -1. */
int qmha_variant_from_name(const char *name);
const char *qmha_variant_name(int variant);
const char *qmha_status_string(int status);
const char *qmha_version(void);
/* Last HIP error string recorded by a failing call on this thread ("" if none). */
const char *qmha_last_error(void);

/*
 * Kernel timing for roofline reporting (bench.py): when enabled, qmha_solve_* record a
 * hipEvent pair around every launch of the dominant ("main") kernel and of the pre-pass.
 * The int8 and fp16 paths split a call into batch chunks whose pre-pass runs on a library
 * stream, overlapped with the previous chunk's main kernel (qmha_set_overlap_chunks, default 1 = off).
 * qmha_profile_collect synchronises those events and returns the summed main-kernel and
 * pre-pass milliseconds and the number of calls since the last collect, then clears the record.
 */
void qmha_profile_enable(int on);
/* Number of batch chunks for the pre-pass / main-kernel overlap (1..16, 1 = off); returns the
 * previous value.  Results are bit-identical for every setting. */
int qmha_set_overlap_chunks(int n);
int qmha_profile_collect(double *main_ms, long long *launches, double *prepass_ms);

/* Release all library-owned workspaces (optional; also released at process exit). */
void qmha_release_workspaces(void);

#ifdef __cplusplus
}
#endif
#endif /* QMHA_LAUNCHERS_H */
