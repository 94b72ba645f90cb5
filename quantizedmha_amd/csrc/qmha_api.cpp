// qmha_api.cpp -- the C-ABI (include/launchers.h): argument checks, workspace ownership,
// variant dispatch, profiling hooks.  Replaces the reference's launch<KernelFn> per-head
// slicer (include/launchers.h:16-72): no per-call cudaMalloc/cudaFree, no extract/concat
// copies (kernels read and write the strided [N, d_model] head slices directly), all B*H
// heads in one grid, and errors are reported instead of ignored.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "../../include/launchers.h"
#include "qmha_kernels.hpp"

#define QMHA_VERSION_STRING "qmha-mi355x 0.1.0 (gfx950)"

namespace {

thread_local std::string g_last_error;

int fail(int status, std::string why) {
    g_last_error = std::move(why);
    return status;
}
int hip_fail(hipError_t e, const char* what) { return fail(QMHA_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e)); }

#define QMHA_HIP_TRY(expr, what)                 \
    do {                                         \
        hipError_t _e = (expr);                  \
        if (_e != hipSuccess) return hip_fail(_e, what); \
    } while (0)

// ---- the variants: one row each, read by every name / size / head-size question below ----
// A head-size mask has bit d / 32 set for every built d (d % 32 == 0, d <= 256).
template <class... T>
constexpr unsigned d_mask(T... d) {
    return (0u | ... | (1u << (d / 32)));
}
constexpr unsigned kEveryD = d_mask(32, 64, 96, 128, 160, 192, 224, 256), kTunedD = d_mask(32, 64, 128);

struct VariantRow {
    int id;
    const char* name;
    size_t (*ws_bytes)(int B, int N, int H, int D);  // nullptr: no scratch
    unsigned plain;                                  // built head sizes of a square call without flags
    // built head sizes of the masked templates (qmha_fa_masked.hip): causal, rectangular and grouped-query calls and
    // the K/V cache are all instances of them and so are built together
    unsigned masked;
};
constexpr VariantRow kVariants[] = {
    {QMHA_FA, "fa", nullptr, kEveryD, 0},
    {QMHA_FA_TC_V1A, "fa_tc_v1a", qmha::f16_workspace_bytes, kEveryD, d_mask(64, 128)},
    {QMHA_FA_TC_INT8_B, "fa_tc_int8_b", [](int B, int N, int H, int D) { return qmha::int8_workspace_bytes(B, N, H, D); },
     kEveryD, kTunedD},
    {QMHA_UNFUSED, "unfused", qmha::unfused_workspace_bytes, kEveryD, 0},
    {QMHA_FA_MFMA, "fa_mfma", nullptr, kEveryD, 0},
    {QMHA_FA_TC_INT8_PT, "fa_tc_int8_pt", qmha::int8_pt_workspace_bytes, kTunedD, 0},  // no reference counterpart
};

const VariantRow* find_variant(int id) {
    for (const VariantRow& r : kVariants)
        if (r.id == id) return &r;
    return nullptr;
}

bool built(unsigned mask, int D) { return D > 0 && D <= 256 && D % 32 == 0 && ((mask >> (D / 32)) & 1u); }

std::string d_list(unsigned mask) {  // "32, 64, 128"
    std::string s;
    for (int d = 32; d <= 256; d += 32)
        if (built(mask, d)) s += (s.empty() ? "" : ", ") + std::to_string(d);
    return s;
}

size_t workspace_bytes(int B, int N, int H, int D, int variant) {
    const VariantRow* v = find_variant(variant);
    return v && v->ws_bytes ? v->ws_bytes(B, N, H, D) : 0;
}

// n_name: what the caller's row count is called in the messages (qmha_solve_rect checks Nq and Nk in turn)
int check_shape(const void* Q, const void* K, const void* V, const void* O, int B, int N, int d_model, int h,
                int variant, int* D_out, const char* n_name = "N") {
    if (!Q || !K || !V || !O) return fail(QMHA_ERR_INVALID, "null tensor pointer");
    if (B < 1 || N < 1 || d_model < 1 || h < 1)
        return fail(QMHA_ERR_INVALID, std::string("B, ") + n_name + ", d_model and h must be positive");
    if (d_model % h != 0) return fail(QMHA_ERR_INVALID, "d_model must be divisible by h");  // config.h:27
    // fa_tc_int8_b.cu:422-423 (N % Br), Br = Bc = 32
    if (N % 32 != 0) return fail(QMHA_ERR_INVALID, std::string(n_name) + " must be a multiple of 32");
    const int D = d_model / h;
    const VariantRow* v = find_variant(variant);
    if (!v) return fail(QMHA_ERR_INVALID, "unknown variant");
    // config.h:32: static_assert(d % 32 == 0)
    if (D % 32 != 0) return fail(QMHA_ERR_INVALID, "head size d = d_model/h must be a multiple of 32");
    // the reference has no upper bound; here the int8 magic-biased accumulator's range
    if (D > 256) return fail(QMHA_ERR_NOSYS, "head size d = d_model/h above 256 is not built");
    if (!built(v->plain, D))
        return fail(QMHA_ERR_NOSYS, std::string(v->name) + " is built for d = " + d_list(v->plain) + " only");
    if ((size_t)B * N * d_model > (size_t)INT32_MAX * 4) return fail(QMHA_ERR_INVALID, "tensor too large");
    *D_out = D;
    return QMHA_OK;
}

// the flags of qmha_solve_opts and every later entry point: unknown bits are invalid
int check_flag_bits(unsigned flags) {
    const unsigned unknown = flags & ~(unsigned)QMHA_FLAG_CAUSAL;
    return unknown ? fail(QMHA_ERR_INVALID, "unknown flag bits " + std::to_string(unknown)) : QMHA_OK;
}

// "<feature> is not built for variant X at d = D (<who has it>)" unless the table's `masked` column has D
int not_built(const char* feature, int variant, int D) {
    if (built(find_variant(variant)->masked, D)) return QMHA_OK;
    std::string have;
    for (const VariantRow& r : kVariants)
        if (r.masked) have += (have.empty() ? "" : "; ") + std::string(r.name) + ": d = " + d_list(r.masked);
    return fail(QMHA_ERR_NOSYS, std::string(feature) + " is not built for variant " + qmha_variant_name(variant) + " at d = " +
                                    std::to_string(D) + " (" + have + ")");
}
constexpr const char* kGroupedFeature = "grouped-query attention (h_kv < h)";

// 1 <= h_kv <= h, h % h_kv == 0 (h >= 1 was checked)
int check_kv_heads(int h, int h_kv) {
    if (h_kv < 1 || h_kv > h || h % h_kv != 0)
        return fail(QMHA_ERR_INVALID, "h_kv must divide h and lie in 1..h (h = " + std::to_string(h) + ", h_kv = " +
                                          std::to_string(h_kv) + ")");
    return QMHA_OK;
}

// One call of any solve entry point.  Q and O are [B, Nq, d_model], K and V [B, Nk, h_kv * d]; the entry points
// without an Nk or an h_kv fill in Nq and h (`square`: their one row count is called N in the messages).
struct Call {
    const float *Q, *K, *V;
    float* O;
    int B, Nq, Nk, d_model, h, h_kv, variant;
    unsigned flags;
    bool square;
    bool caller_owned;  // scratch is the caller's ws_bytes at ws (the slot is leased all the same), else the slot's own
    void* ws;
    size_t ws_bytes;
};

// Every check of a call but its workspace's size, run once and before any HIP call.  The order decides which
// error a call that is wrong in several ways reports (tests/test_hostpath_cpu.py).
int check_call(const Call& c, int* D) {
    int st = check_shape(c.Q, c.K, c.V, c.O, c.B, c.Nq, c.d_model, c.h, c.variant, D, c.square ? "N" : "Nq");
    if (st == QMHA_OK) st = check_shape(c.Q, c.K, c.V, c.O, c.B, c.Nk, c.d_model, c.h, c.variant, D, c.square ? "N" : "Nk");
    if (st == QMHA_OK) st = check_kv_heads(c.h, c.h_kv);
    if (st == QMHA_OK) st = check_flag_bits(c.flags);
    if (st != QMHA_OK) return st;
    const bool causal = c.flags & QMHA_FLAG_CAUSAL;
    if (causal && c.Nq > c.Nk)
        return fail(QMHA_ERR_INVALID, "causal attention is bottom-right aligned and needs Nk >= Nq (Nq = " +
                                          std::to_string(c.Nq) + ", Nk = " + std::to_string(c.Nk) + ")");
    // the kind of call names the feature; all three are the masked templates
    if (c.h_kv < c.h) return not_built(kGroupedFeature, c.variant, *D);
    if (c.Nq != c.Nk) return not_built("rectangular attention (Nq != Nk)", c.variant, *D);
    return causal ? not_built("causal attention", c.variant, *D) : QMHA_OK;
}

// ---- profiling --------------------------------------------------------------------------
// Per call: event pairs around every pre-pass launch (on the pre-pass stream) and every main
// launch (on the caller's stream); qmha_profile_collect sums them per call.
using Marks = std::vector<std::pair<hipEvent_t, hipEvent_t>>;
struct ProfRec {
    Marks pre, main;
};
std::mutex g_prof_mu;
bool g_prof_on = false;
std::vector<ProfRec> g_prof_recs;
std::vector<hipEvent_t> g_event_pool;

bool profiling_on() {
    std::lock_guard<std::mutex> lk(g_prof_mu);
    return g_prof_on;
}
void keep_record(ProfRec&& rec) {
    std::lock_guard<std::mutex> lk(g_prof_mu);
    g_prof_recs.push_back(std::move(rec));
}

hipEvent_t take_event() {
    if (!g_event_pool.empty()) {
        hipEvent_t e = g_event_pool.back();
        g_event_pool.pop_back();
        return e;
    }
    hipEvent_t e = nullptr;
    if (hipEventCreate(&e) != hipSuccess) return nullptr;
    return e;
}

// one profiling event recorded on `s`: it opens a new pair of `v` (begin) or closes the last one
int mark(Marks& v, hipStream_t s, bool begin) {
    hipEvent_t e;
    {
        std::lock_guard<std::mutex> lk(g_prof_mu);
        e = take_event();
    }
    if (!e) return fail(QMHA_ERR_HIP, "hipEventCreate failed");
    if (begin) v.push_back({e, nullptr});
    else v.back().second = e;
    QMHA_HIP_TRY(hipEventRecord(e, s), "hipEventRecord");
    return QMHA_OK;
}

// enqueue one launch on `s`, between a pair of profiling events when `marks` is given
template <class Launch>
int timed(Marks* marks, hipStream_t s, const char* what, Launch&& launch) {
    int st = marks ? mark(*marks, s, true) : QMHA_OK;
    if (st != QMHA_OK) return st;
    QMHA_HIP_TRY(launch(), what);
    return marks ? mark(*marks, s, false) : QMHA_OK;
}

// ---- library-owned per-stream state, one slot per (device, stream) ---------------------
// Threading contract: any number of host threads may call every entry point at once.
// The reference gets that from per-call cudaMalloc'd scratch and private streams (include/launchers.h:
// 27-33, freed at :64-71); here the scratch and the overlap side stream are cached, so a call LEASES its
// (device, stream) slot: the slot's mutex is held from before the call's first HIP call until its last
// kernel has been enqueued, and nothing in a slot is touched outside its lease.  Calls on one stream
// therefore enqueue one whole call after another (pre-pass and main kernel of a call are never separated
// by another call's pre-pass), and the stream runs them in that order.  Calls on different streams use
// different slots.  hipStreamPerThread names a different stream in every thread, so its slot key carries
// the thread id.  A slot that must grow never frees the buffer other enqueued work may still read: the
// old buffer is retired behind an event recorded on the slot's stream and freed once that event has
// completed (checked at the slot's next lease for scratch, or at release).
struct WsKey {
    int dev;
    void* stream;
    std::thread::id tid;  // hipStreamPerThread only
    bool operator<(const WsKey& o) const {
        if (dev != o.dev) return dev < o.dev;
        if (stream != o.stream) return stream < o.stream;
        return tid < o.tid;
    }
};
struct WsSlot {
    std::mutex lease;  // held across a call's enqueue
    void* ptr = nullptr;
    size_t bytes = 0;
    std::vector<std::pair<void*, hipEvent_t>> retired;  // grown-out buffers, freed once their event completed
    // pre-pass / main-kernel overlap (run_chunked), created at the first call with more than one chunk
    hipStream_t side = nullptr;
    hipEvent_t start = nullptr;
    std::vector<hipEvent_t> ready;  // one per chunk
};
std::mutex g_ws_mu;  // guards the map only (slots are never erased); never held while waiting for a lease by a caller
std::map<WsKey, std::unique_ptr<WsSlot>> g_ws;

// free the retired buffers whose last reader has completed (all when `wait`); caller holds the lease
void reap_retired(WsSlot& s, bool wait) {
    auto it = s.retired.begin();
    while (it != s.retired.end()) {
        if (wait) (void)hipEventSynchronize(it->second);
        else if (hipEventQuery(it->second) != hipSuccess) {
            ++it;
            continue;
        }
        (void)hipEventDestroy(it->second);
        (void)hipFree(it->first);
        it = s.retired.erase(it);
    }
}

// A held slot: slot and buffer stay this call's until the lease is destroyed (after the last enqueue).
struct WsLease {
    std::unique_lock<std::mutex> lk;
    WsSlot* slot = nullptr;
    void* ptr = nullptr;  // >= `need` bytes (nullptr for need == 0: a call that brings its own scratch, or none)
};

int lease_workspace(size_t need, hipStream_t stream, WsLease* out) {
    out->ptr = nullptr;
    int dev = 0;
    QMHA_HIP_TRY(hipGetDevice(&dev), "hipGetDevice");
    {
        std::lock_guard<std::mutex> lk(g_ws_mu);
        const WsKey key{dev, (void*)stream, stream == hipStreamPerThread ? std::this_thread::get_id() : std::thread::id()};
        std::unique_ptr<WsSlot>& sp = g_ws[key];
        if (!sp) sp.reset(new WsSlot);
        out->slot = sp.get();
    }
    out->lk = std::unique_lock<std::mutex>(out->slot->lease);
    WsSlot& s = *out->slot;
    if (need == 0) return QMHA_OK;  // no HIP call beyond hipGetDevice: qmha_solve_ws stays capturable in a graph
    if (!s.retired.empty()) reap_retired(s, false);
    if (s.bytes < need) {
        if (s.ptr) {
            // work already enqueued on this stream may still read the old buffer: retire it behind an event
            hipEvent_t ev = nullptr;
            QMHA_HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming), "hipEventCreate");
            const hipError_t e = hipEventRecord(ev, stream);
            if (e != hipSuccess) {
                (void)hipEventDestroy(ev);
                return hip_fail(e, "hipEventRecord");
            }
            s.retired.emplace_back(s.ptr, ev);
            s.ptr = nullptr;
            s.bytes = 0;
        }
        const size_t alloc = qmha::align_up(need + need / 8, 1 << 20);
        if (hipMalloc(&s.ptr, alloc) != hipSuccess) {
            s.ptr = nullptr;
            return fail(QMHA_ERR_NOMEM, "hipMalloc of workspace failed");
        }
        s.bytes = alloc;
    }
    out->ptr = s.ptr;
    return QMHA_OK;
}

// ---- pre-pass / main-kernel overlap (int8 and fp16 paths) ------------------------------
// The HBM-bound pre-pass (quantise / convert) of batch chunk c+1 runs on the slot's side stream
// while the compute-bound main kernel of chunk c runs on the caller's stream.
// Chunks are disjoint slices of the same workspace arrays, so only "pre(c) before main(c)"
// and "previous call done before pre(0)" need ordering.  QMHA_OVERLAP_CHUNKS (default 1 =
// off: measured slower at C4, the co-running pre-pass slows the main kernel more than it hides,
// profiles/r01/overlap_sweep.txt) sets the number of chunks.
constexpr int kMaxChunks = 16;
std::atomic<int> g_overlap_chunks{-1};  // -1: not yet read from QMHA_OVERLAP_CHUNKS

int clamp_chunks(int c) { return c < 1 ? 1 : (c > kMaxChunks ? kMaxChunks : c); }

int overlap_chunks(int B) {
    int c = g_overlap_chunks.load();
    if (c < 0) {
#ifdef QMHA_ABLATION  // profiling builds: QMHA_OVERLAP_CHUNKS sets the default (production: the API only)
        const char* e = std::getenv("QMHA_OVERLAP_CHUNKS");
        c = clamp_chunks(e ? std::atoi(e) : 1);
#else
        c = 1;
#endif
        g_overlap_chunks.store(c);
    }
    return c > B ? B : c;
}

// the slot's side stream with `nchunks` ready events; caller holds the lease
int ensure_side(WsSlot& s, int nchunks) {
    if (!s.side) QMHA_HIP_TRY(hipStreamCreateWithFlags(&s.side, hipStreamNonBlocking), "hipStreamCreate");
    if (!s.start) QMHA_HIP_TRY(hipEventCreateWithFlags(&s.start, hipEventDisableTiming), "hipEventCreate");
    while ((int)s.ready.size() < nchunks) {
        hipEvent_t e = nullptr;
        QMHA_HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming), "hipEventCreate");
        s.ready.push_back(e);
    }
    return QMHA_OK;
}

struct Chunk {  // sequences [b0, b0 + nb) of the batch
    size_t b0;
    int nb;
};

// A call of a chunked variant: pre(chunk, s) / main(chunk) enqueue one chunk's pre-pass on stream s / its
// main kernel on the caller's stream.  Every pre-pass is enqueued first (the side stream runs ahead).
template <class Pre, class Main>
int run_chunked(int B, hipStream_t stream, WsSlot& slot, Marks* pre_m, Marks* main_m, const char* pre_what, Pre&& pre,
                const char* main_what, Main&& main) {
    const int nc = overlap_chunks(B);
    hipStream_t pre_s = stream;
    if (nc > 1) {
        int st = ensure_side(slot, nc);
        if (st != QMHA_OK) return st;
        QMHA_HIP_TRY(hipEventRecord(slot.start, stream), "hipEventRecord");
        QMHA_HIP_TRY(hipStreamWaitEvent(slot.side, slot.start, 0), "hipStreamWaitEvent");
        pre_s = slot.side;
    }
    Chunk ch[kMaxChunks];
    for (int c = 0; c < nc; ++c) {
        const long long b0 = (long long)B * c / nc, b1 = (long long)B * (c + 1) / nc;
        ch[c] = Chunk{(size_t)b0, (int)(b1 - b0)};
        int st = timed(pre_m, pre_s, pre_what, [&] { return pre(ch[c], pre_s); });
        if (st != QMHA_OK) return st;
        if (nc > 1) QMHA_HIP_TRY(hipEventRecord(slot.ready[c], pre_s), "hipEventRecord");
    }
    for (int c = 0; c < nc; ++c) {
        if (nc > 1) QMHA_HIP_TRY(hipStreamWaitEvent(stream, slot.ready[c], 0), "hipStreamWaitEvent");
        int st = timed(main_m, stream, main_what, [&] { return main(ch[c]); });
        if (st != QMHA_OK) return st;
    }
    return QMHA_OK;
}

qmha::Int8Workspace int8_slice(qmha::Int8Workspace w, size_t b0, int N, int H, int D) {
    const size_t e = b0 * H * N * D, g = b0 * H * (N / 32);  // 32-row quantisation groups
    w.Ki += e, w.Vh += e, w.sK += g, w.sV += g;
    return w;
}
qmha::F16Workspace f16_slice(qmha::F16Workspace w, size_t b0, int N, int H, int D) {
    const size_t e = b0 * H * N * D;
    w.Kh += e, w.Vt += e;
    return w;
}

// Enqueue one checked call on `stream`; `ws` holds workspace_bytes(...) bytes and `slot` is leased by the caller.
// Q and O have Nq rows, K and V have N; the pre-passes and the workspaces see K and V only, so they follow N.
// A causal, rectangular (Nq != N) or grouped (h_kv < h: the pre-pass runs with h_kv heads) call -- check_call passed:
// int8 / fp16 at a head size of the `masked` column -- takes the masked main kernels (qmha::launch_fa_masked); a
// plain square call keeps the non-causal ones.
int run(const Call& call, void* ws, WsSlot& slot, hipStream_t stream) {
    const float *Q = call.Q, *K = call.K, *V = call.V;
    float* O = call.O;
    const int B = call.B, Nq = call.Nq, N = call.Nk, d_model = call.d_model, h = call.h, h_kv = call.h_kv, variant = call.variant;
    const int D = d_model / h;
    const bool causal = call.flags & QMHA_FLAG_CAUSAL;
    const bool rect = Nq != N, gqa = h_kv < h;
    const bool masked = causal || rect || gqa;
    const int kv_model = h_kv * D;  // row width of K and V
    const auto masked_call = [&](int nb) { return qmha::MaskedCall{nb, Nq, N, h, h_kv, D, d_model, causal, -1, nullptr}; };
    const bool prof = profiling_on();
    ProfRec rec;
    Marks *pre_m = prof ? &rec.pre : nullptr, *main_m = prof ? &rec.main : nullptr;
    const size_t slab = (size_t)N * kv_model, qslab = (size_t)Nq * d_model;  // floats per sequence: K and V, Q and O
    int st;
    switch (variant) {
        case QMHA_FA_TC_INT8_B: {
            const qmha::Int8Workspace w8 = qmha::int8_carve(ws, B, N, h_kv, D);
            st = run_chunked(
                B, stream, slot, pre_m, main_m, "quant_int8 launch",
                [&](Chunk c, hipStream_t s) {
                    const qmha::Int8Workspace w = int8_slice(w8, c.b0, N, h_kv, D);
                    return qmha::launch_quant_int8(Q + c.b0 * qslab, K + c.b0 * slab, V + c.b0 * slab, w, w.Vh, /*v_mode=*/1,
                                                   c.nb, N, h_kv, D, kv_model, s, /*first_tensor=*/1);
                },
                gqa ? "fa_int8 gqa launch" : rect ? "fa_int8 rect launch" : causal ? "fa_int8 causal launch" : "fa_int8 launch",
                [&](Chunk c) {
                    const qmha::Int8Workspace w = int8_slice(w8, c.b0, N, h_kv, D);
                    const float* q = Q + c.b0 * qslab;
                    float* o = O + c.b0 * qslab;
                    return masked ? qmha::launch_fa_masked(w, q, o, masked_call(c.nb), stream)
                                  : qmha::launch_fa_int8_main(w, q, o, c.nb, N, h, D, d_model, stream);
                });
            break;
        }
        case QMHA_FA_TC_V1A: {
            const qmha::F16Workspace w16 = qmha::f16_carve(ws, B, N, h_kv, D);
            st = run_chunked(
                B, stream, slot, pre_m, main_m, "convert_f16 launch",
                [&](Chunk c, hipStream_t s) {
                    return qmha::launch_convert_f16(Q + c.b0 * qslab, K + c.b0 * slab, V + c.b0 * slab,
                                                    f16_slice(w16, c.b0, N, h_kv, D), c.nb, N, h_kv, D, kv_model, s);
                },
                gqa ? "fa_f16 gqa launch" : rect ? "fa_f16 rect launch" : causal ? "fa_f16 causal launch" : "fa_f16 launch",
                [&](Chunk c) {
                    const qmha::F16Workspace w = f16_slice(w16, c.b0, N, h_kv, D);
                    const float* q = Q + c.b0 * qslab;
                    float* o = O + c.b0 * qslab;
                    return masked ? qmha::launch_fa_masked(w, q, o, masked_call(c.nb), stream)
                                  : qmha::launch_fa_f16_main(w, q, o, c.nb, N, h, D, d_model, stream);
                });
            break;
        }
        case QMHA_FA_TC_INT8_PT: {
            // per-tensor mode: group absmax of Q, K, V + K/V quantisation with the head-slice scales
            // (two pre-pass launches), then the main kernel (Q quantised in registers)
            const qmha::Int8Workspace w = qmha::int8_pt_carve(ws, B, N, h, D);
            st = timed(pre_m, stream, "quant_int8_pt launch",
                       [&] { return qmha::launch_quant_int8_pt(Q, K, V, w, B, N, h, D, d_model, stream); });
            if (st == QMHA_OK)
                st = timed(main_m, stream, "fa_int8_pt launch",
                           [&] { return qmha::launch_fa_int8_pt_main(w, Q, O, B, N, h, D, d_model, stream); });
            break;
        }
        case QMHA_FA:
        case QMHA_FA_MFMA:
            st = timed(main_m, stream, "fa_f32 launch",
                       [&] { return qmha::launch_fa_f32(Q, K, V, O, B, N, h, D, d_model, variant == QMHA_FA_MFMA, stream); });
            break;
        case QMHA_UNFUSED:
            st = timed(main_m, stream, "unfused launch",
                       [&] { return qmha::launch_unfused(Q, K, V, O, ws, B, N, h, D, d_model, stream); });
            break;
        default: return fail(QMHA_ERR_INVALID, "unknown variant");
    }
    if (st == QMHA_OK && prof) keep_record(std::move(rec));
    return st;
}

// The one solve path behind every qmha_solve_* entry point: check_call (before any HIP call), the slot's lease held
// until the last kernel is enqueued, run().  The scratch is that of the keys: workspace_bytes(B, Nk, h_kv, ...).  A
// caller workspace leases the slot all the same (need == 0): the overlap side stream lives there.
int solve_on(const Call& c, void* stream_) {
    const hipStream_t stream = (hipStream_t)stream_;
    int D = 0;
    int st = check_call(c, &D);
    if (st != QMHA_OK) return st;
    const size_t need = workspace_bytes(c.B, c.Nk, c.h_kv, D, c.variant);
    if (c.caller_owned && c.ws_bytes < need) return fail(QMHA_ERR_INVALID, "workspace too small");
    WsLease lease;
    st = lease_workspace(c.caller_owned ? 0 : need, stream, &lease);
    if (st != QMHA_OK) return st;
    return run(c, c.caller_owned ? c.ws : lease.ptr, *lease.slot, stream);
}

// The debug hooks' skeleton: `need` bytes of the null stream's slot, body(ws) enqueues the pre-pass and the
// dumping kernel there, then the lease is dropped and the stream waited for (the hooks are blocking).
template <class Body>
int debug_run(size_t need, Body&& body) {
    WsLease lease;
    int st = lease_workspace(need, nullptr, &lease);
    if (st != QMHA_OK) return st;
    st = body(lease.ptr);
    if (st != QMHA_OK) return st;
    lease.lk.unlock();
    QMHA_HIP_TRY(hipStreamSynchronize(nullptr), "hipStreamSynchronize");
    return QMHA_OK;
}

}  // namespace

// ---- persistent K/V cache ---------------------------------------------------------
// A host object over caller-owned device memory laid out as the variant's workspace carve at N = cap.  No HIP
// allocation, no synchronisation, no leased slot (there is no scratch): `mu` is held across each enqueue, and the
// caller orders the operations on one cache (one stream, or its own events).
struct qmha_kv_cache {
    std::mutex mu;
    void* mem;
    int B, cap, d_model, h, D, variant;
    int h_kv;  // K/V heads: the memory is the variant's carve at H = h_kv (== h unless created by _create_gqa)
    int len;   // valid rows of every head slice
    // the raw rows of each sequence's open group (qmha_kv_cache_attach_tail; int8 only), caller-owned like `mem`
    void* tail = nullptr;
    // a paged cache (qmha_kv_cache_create_paged): `mem` is a pool of num_pages pages of page_rows rows --
    // the variant's carve at B := num_pages, N := page_rows --, cap the logical capacity max_pages * page_rows of a
    // sequence, B the sequence slots (the tail's).  num_pages == 0: a contiguous cache.
    int num_pages = 0, page_rows = 0, max_pages = 0;
    bool paged() const { return num_pages > 0; }
    qmha::PageTable pages(const int32_t* table) const { return {table, page_rows, max_pages, num_pages}; }
};

namespace {

// f(the cache's memory as its variant's workspace); the one place that knows the precision of a cache
template <class F>
hipError_t with_carve(const qmha_kv_cache& c, F&& f) {
    const int slices = c.paged() ? c.num_pages : c.B, rows = c.paged() ? c.page_rows : c.cap;
    return c.variant == QMHA_FA_TC_INT8_B ? f(qmha::int8_carve(c.mem, slices, rows, c.h_kv, c.D))
                                          : f(qmha::f16_carve(c.mem, slices, rows, c.h_kv, c.D));
}

// One operation on a cache, after the checks that need no lock: `mu` held across check(len) -- the checks against the
// valid rows -- and the enqueue of launch(workspace, len) on `stream`, timed on the record's `marks` list when profiling
template <class Check, class Launch>
int cache_enqueue(qmha_kv_cache* c, Marks ProfRec::*marks, void* stream, const char* what, Check&& check, Launch&& launch) {
    std::lock_guard<std::mutex> lk(c->mu);
    const int len = c->len;
    int st = check(len);
    if (st != QMHA_OK) return st;
    const bool prof = profiling_on();
    ProfRec rec;
    st = timed(prof ? &(rec.*marks) : nullptr, (hipStream_t)stream, what,
               [&] { return with_carve(*c, [&](const auto& w) { return launch(w, len); }); });
    if (st == QMHA_OK && prof) keep_record(std::move(rec));
    return st;
}
const auto kNoLenCheck = [](int) { return QMHA_OK; };

// the entry points of one kind of cache refuse the other kind
int check_cache_kind(const qmha_kv_cache* c, bool paged_call, const char* what) {
    if (c->paged() == paged_call) return QMHA_OK;
    return fail(QMHA_ERR_INVALID, std::string(what) + (paged_call ? ": the cache is contiguous (qmha_kv_cache_create): the paged entry points "
                                                                    "need a cache of qmha_kv_cache_create_paged"
                                                                  : ": the cache is paged (qmha_kv_cache_create_paged): use "
                                                                    "qmha_kv_cache_append_paged / qmha_attend_cached_paged"));
}

// One token-granular call on a cache: the entry point's name in messages, and whether it is one of the
// paged kind (then `table` is an argument and cap reads "max_pages * page_rows").  Each check of these entry points is
// written once here; an entry point strings them in the order they win.
struct CacheCall {
    qmha_kv_cache* c;
    const char* what;
    bool paged;
    int bad(const std::string& why) const { return fail(QMHA_ERR_INVALID, std::string(what) + ": " + why); }
    std::string cap() const { return std::string("cap = ") + (paged ? "max_pages * page_rows = " : "") + std::to_string(c->cap); }
    std::string label() const { return std::string("kv_cache ") + what + " launch"; }
    // the cache, its kind and the call's two tensors
    int operands(const void* a, const void* b) const {
        if (!c) return fail(QMHA_ERR_INVALID, "null cache");
        if (int ck = check_cache_kind(c, paged, what)) return ck;
        if (!a || !b) return fail(QMHA_ERR_INVALID, "null tensor pointer");
        return QMHA_OK;
    }
    // a device array: `name` is "pos (a device int32[B])"
    int words(const int32_t* p, const char* name) const { return p ? (int)QMHA_OK : bad(std::string("null ") + name); }
    int table(const int32_t* t) const { return paged ? words(t, "table (a device int32[B][max_pages])") : (int)QMHA_OK; }
    // an attend's lens, table and flags
    int attend_words(const int32_t* lens, const int32_t* t, unsigned flags) const {
        if (int st = words(lens, "lens (a device int32[B])")) return st;
        if (int st = table(t)) return st;
        if (flags != QMHA_FLAG_CAUSAL) return bad("flags must be QMHA_FLAG_CAUSAL (the kernels have no mask but the diagonal)");
        return QMHA_OK;
    }
    // a row count every sequence shares (n, Nq): 1 <= rows <= cap
    int rows(const char* name, int n) const {
        if (n >= 1 && n <= c->cap) return QMHA_OK;
        return bad(std::string(name) + " = " + std::to_string(n) + " rows, needs 1 <= " + name + " <= " + cap());
    }
    // a sliding window: whole 32-row tiles, at least one
    int window(int w) const {
        if (w >= 32 && w % 32 == 0) return QMHA_OK;
        return bad("window = " + std::to_string(w) + " rows, needs a multiple of 32 with window >= 32 (the window's left edge falls on a "
                   "32-row key tile's diagonal)");
    }
    // a packed call's rows and the bound its grid is sized for: 1 <= bound <= min(total, cap)
    int bound(const char* name, int total, int b) const {
        if (total < 1) return bad("total = " + std::to_string(total) + " rows, needs total >= 1");
        if (b >= 1 && b <= total && b <= c->cap) return QMHA_OK;
        return bad(std::string(name) + " = " + std::to_string(b) + ", needs 1 <= " + name + " <= min(total = " + std::to_string(total) + ", " +
                   cap() + ")");
    }
    // an append, under the mutex (attach_tail writes `tail` under it)
    int tail() const {
        if (c->variant == QMHA_FA_TC_INT8_B && !c->tail) return bad("an int8 cache needs its tail (qmha_kv_cache_attach_tail)");
        return QMHA_OK;
    }
    // the token-granular attend's call, over the cache's pages when it has some (Nq: the rows, or a packed call's bound)
    qmha::MaskedCall attend(int Nq, const int32_t* lens, const int32_t* t) const {
        return {c->B, Nq, c->cap, c->h, c->h_kv, c->D, c->d_model, true, -1, lens, true, c->pages(t)};
    }
};

// The uniform-count append (qmha_kv_cache_append_tokens / _paged): `table` null is the contiguous one
int append_rows(const CacheCall& k, const float* K, const float* V, int n, const int32_t* pos, const int32_t* table, void* stream) {
    if (int st = k.operands(K, V)) return st;
    if (int st = k.words(pos, "pos (a device int32[B])")) return st;
    if (int st = k.table(table)) return st;
    if (int st = k.rows("n", n)) return st;
    const qmha_kv_cache* c = k.c;
    return cache_enqueue(
        k.c, &ProfRec::pre, stream, k.label().c_str(), [&](int) { return k.tail(); },
        [&](const auto& w, int) {
            return qmha::launch_kv_tokens(K, V, w, static_cast<float*>(c->tail), c->B, n, c->cap, pos, c->h_kv, c->D, c->h_kv * c->D,
                                          (hipStream_t)stream, c->pages(table));
        });
}

// The uniform-count attend (qmha_attend_cached_tokens / _paged); window non-null: its windowed form (_tokens_window /
// _paged_window)
int attend_rows(const CacheCall& k, const float* Q, float* O, int Nq, const int32_t* lens, const int32_t* table, unsigned flags,
                void* stream, const int* window = nullptr) {
    if (int st = k.operands(Q, O)) return st;
    if (int st = k.attend_words(lens, table, flags)) return st;
    if (int st = k.rows("Nq", Nq)) return st;
    if (window) {
        if (int st = k.window(*window)) return st;
    }
    return cache_enqueue(k.c, &ProfRec::main, stream, k.label().c_str(), kNoLenCheck, [&](const auto& w, int) {
        if (window) return qmha::launch_fa_window(w, Q, O, k.attend(Nq, lens, table), *window, (hipStream_t)stream);
        return qmha::launch_fa_masked(w, Q, O, k.attend(Nq, lens, table), (hipStream_t)stream);
    });
}

}  // namespace

int qmha::tune_config(const char* env_name) {
    static std::mutex mu;
    static std::map<std::string, int> cache;
    std::lock_guard<std::mutex> lk(mu);
    auto it = cache.find(env_name);
    if (it != cache.end()) return it->second;
    int v = 0;
    if (const char* e = std::getenv(env_name)) {
        int w = 0, sg = 0;
        if (std::sscanf(e, "%dx%d", &w, &sg) == 2 && w > 0 && w < 10 && sg > 0 && sg < 10) {
            v = w * 10 + sg;  // "WAVESxSG"
        } else if (std::sscanf(e, "%d", &w) == 1 && w > 0) {
            v = w;  // a kernel-specific numeric geometry code
        }
    }
    cache[env_name] = v;
    return v;
}

extern "C" {

int qmha_solve_ws(const float* Q, const float* K, const float* V, float* O, int B, int N, int d_model, int h,
                  int variant, void* workspace, size_t workspace_bytes_, void* stream) {
    // always the caller's scratch: a null one holds no bytes, whatever size is claimed
    return solve_on({Q, K, V, O, B, N, N, d_model, h, h, variant, 0, true, true, workspace, workspace ? workspace_bytes_ : 0},
                    stream);
}

int qmha_solve_ex(const float* Q, const float* K, const float* V, float* O, int B, int N, int d_model, int h,
                  int variant, void* stream) {
    return solve_on({Q, K, V, O, B, N, N, d_model, h, h, variant, 0, true, false, nullptr, 0}, stream);
}

// _opts, _rect and _gqa: a null workspace is the library's scratch
int qmha_solve_opts(const float* Q, const float* K, const float* V, float* O, int B, int N, int d_model, int h,
                    int variant, unsigned flags, void* workspace, size_t workspace_bytes_, void* stream) {
    return solve_on({Q, K, V, O, B, N, N, d_model, h, h, variant, flags, true, workspace != nullptr, workspace, workspace_bytes_},
                    stream);
}

int qmha_solve_rect(const float* Q, const float* K, const float* V, float* O, int B, int Nq, int Nk, int d_model, int h,
                    int variant, unsigned flags, void* workspace, size_t workspace_bytes_, void* stream) {
    return solve_on({Q, K, V, O, B, Nq, Nk, d_model, h, h, variant, flags, false, workspace != nullptr, workspace, workspace_bytes_},
                    stream);
}

int qmha_solve_gqa(const float* Q, const float* K, const float* V, float* O, int B, int Nq, int Nk, int d_model, int h,
                   int h_kv, int variant, unsigned flags, void* workspace, size_t workspace_bytes_, void* stream) {
    return solve_on({Q, K, V, O, B, Nq, Nk, d_model, h, h_kv, variant, flags, false, workspace != nullptr, workspace,
                     workspace_bytes_},
                    stream);
}

size_t qmha_workspace_size(int B, int N, int d_model, int h, int variant) {
    if (B < 1 || N < 1 || h < 1 || d_model % h) return 0;
    return workspace_bytes(B, N, h, d_model / h, variant);
}

// ---- persistent K/V cache: every check runs before any HIP call -------------------------------------
size_t qmha_kv_cache_bytes(int B, int cap, int d_model, int h, int variant) {
    return qmha_workspace_size(B, cap, d_model, h, variant);  // the variant's carve at N = cap
}

int qmha_kv_cache_create_gqa(qmha_kv_cache_t** out, void* mem, size_t bytes, int B, int cap, int d_model, int h, int h_kv,
                             int variant) {
    if (!out) return fail(QMHA_ERR_INVALID, "null cache handle pointer");
    *out = nullptr;
    if (!mem) return fail(QMHA_ERR_INVALID, "null cache memory");
    int D = 0;
    int st = check_shape(mem, mem, mem, mem, B, cap, d_model, h, variant, &D, "cap");  // cap >= 32, cap % 32 == 0
    if (st == QMHA_OK) st = check_kv_heads(h, h_kv);
    if (st == QMHA_OK) st = not_built(h_kv < h ? kGroupedFeature : "the persistent K/V cache", variant, D);
    if (st != QMHA_OK) return st;
    if (reinterpret_cast<uintptr_t>(mem) % 256 != 0) return fail(QMHA_ERR_INVALID, "cache memory must be 256-byte aligned");
    const size_t need = workspace_bytes(B, cap, h_kv, D, variant);
    if (bytes < need)
        return fail(QMHA_ERR_INVALID, "cache memory too small: " + std::to_string(bytes) + " bytes, qmha_kv_cache_bytes is " +
                                          std::to_string(need));
    qmha_kv_cache* c = new qmha_kv_cache;
    c->mem = mem;
    c->B = B, c->cap = cap, c->d_model = d_model, c->h = h, c->D = D, c->variant = variant;
    c->h_kv = h_kv;
    c->len = 0;
    *out = c;
    return QMHA_OK;
}

int qmha_kv_cache_create(qmha_kv_cache_t** out, void* mem, size_t bytes, int B, int cap, int d_model, int h, int variant) {
    return qmha_kv_cache_create_gqa(out, mem, bytes, B, cap, d_model, h, h, variant);
}

void qmha_kv_cache_destroy(qmha_kv_cache_t* c) { delete c; }

int qmha_kv_cache_len(const qmha_kv_cache_t* c) {
    if (!c) return 0;
    std::lock_guard<std::mutex> lk(const_cast<qmha_kv_cache_t*>(c)->mu);
    return c->len;
}

int qmha_kv_cache_truncate(qmha_kv_cache_t* c, int len) {
    if (!c) return fail(QMHA_ERR_INVALID, "null cache");
    if (int ck = check_cache_kind(c, false, "truncate")) return ck;
    std::lock_guard<std::mutex> lk(c->mu);
    if (len < 0 || len % 32 != 0) return fail(QMHA_ERR_INVALID, "truncate: len must be a non-negative multiple of 32");
    if (len > c->len)
        return fail(QMHA_ERR_INVALID, "truncate: len = " + std::to_string(len) + " is above the cache's " +
                                          std::to_string(c->len) + " valid rows");
    c->len = len;
    return QMHA_OK;
}

int qmha_kv_cache_append(qmha_kv_cache_t* c, const float* K, const float* V, int n, void* stream) {
    if (!c) return fail(QMHA_ERR_INVALID, "null cache");
    if (int ck = check_cache_kind(c, false, "append")) return ck;
    if (!K || !V) return fail(QMHA_ERR_INVALID, "null tensor pointer");
    if (n < 32 || n % 32 != 0) return fail(QMHA_ERR_INVALID, "append: n must be a positive multiple of 32");
    return cache_enqueue(
        c, &ProfRec::pre, stream, "kv_cache append launch",
        [&](int len) {
            if ((long long)len + n > c->cap)
                return fail(QMHA_ERR_INVALID, "append: " + std::to_string(n) + " rows behind len = " + std::to_string(len) +
                                                  " exceed cap = " + std::to_string(c->cap));
            return (int)QMHA_OK;
        },
        [&](const auto& w, int len) {
            const hipError_t e = qmha::launch_kv_append(K, V, w, c->B, n, c->cap, len, nullptr, c->h_kv, c->D, c->h_kv * c->D,
                                                        (hipStream_t)stream);
            if (e == hipSuccess) c->len = len + n;  // the rows are on their way whatever becomes of the closing profile event
            return e;
        });
}

int qmha_attend_cached(qmha_kv_cache_t* c, const float* Q, float* O, int Nq, unsigned flags, void* stream) {
    if (!c) return fail(QMHA_ERR_INVALID, "null cache");
    if (int ck = check_cache_kind(c, false, "attend")) return ck;
    int D = 0;
    int st = check_shape(Q, Q, Q, O, c->B, Nq, c->d_model, c->h, c->variant, &D, "Nq");
    if (st == QMHA_OK) st = check_flag_bits(flags);
    if (st != QMHA_OK) return st;
    const bool causal = flags & QMHA_FLAG_CAUSAL;
    return cache_enqueue(
        c, &ProfRec::main, stream, "kv_cache attend launch",
        [&](int len) {
            if (causal && Nq > len)
                return fail(QMHA_ERR_INVALID, "causal attention is bottom-right aligned and needs len >= Nq (Nq = " +
                                                  std::to_string(Nq) + ", len = " + std::to_string(len) + ")");
            if (!causal && len != c->cap)
                return fail(QMHA_ERR_INVALID, "attention without QMHA_FLAG_CAUSAL reads all cap = " + std::to_string(c->cap) +
                                                  " rows and the cache holds len = " + std::to_string(len) +
                                                  ": the kernel has no unmasked mode that stops before cap");
            return (int)QMHA_OK;
        },
        [&](const auto& w, int len) {
            return qmha::launch_fa_masked(w, Q, O, {c->B, Nq, c->cap, c->h, c->h_kv, c->D, c->d_model, causal, len, nullptr},
                                          (hipStream_t)stream);
        });
}

// ---- per-sequence lengths read on the device: the host `len` is neither read nor changed ----
int qmha_kv_cache_append_at(qmha_kv_cache_t* c, const float* K, const float* V, int n, const int32_t* pos, void* stream) {
    if (!c) return fail(QMHA_ERR_INVALID, "null cache");
    if (int ck = check_cache_kind(c, false, "append_at")) return ck;
    if (!K || !V) return fail(QMHA_ERR_INVALID, "null tensor pointer");
    if (!pos) return fail(QMHA_ERR_INVALID, "append_at: null pos (a device int32[B])");
    if (n < 32 || n % 32 != 0) return fail(QMHA_ERR_INVALID, "append_at: n must be a positive multiple of 32");
    if (n > c->cap)
        return fail(QMHA_ERR_INVALID, "append_at: n = " + std::to_string(n) + " rows exceed cap = " + std::to_string(c->cap));
    return cache_enqueue(c, &ProfRec::pre, stream, "kv_cache append_at launch", kNoLenCheck, [&](const auto& w, int) {
        return qmha::launch_kv_append(K, V, w, c->B, n, c->cap, 0, pos, c->h_kv, c->D, c->h_kv * c->D, (hipStream_t)stream);
    });
}

int qmha_attend_cached_varlen(qmha_kv_cache_t* c, const float* Q, float* O, int Nq, const int32_t* lens, unsigned flags,
                              void* stream) {
    if (!c) return fail(QMHA_ERR_INVALID, "null cache");
    if (int ck = check_cache_kind(c, false, "attend_varlen")) return ck;
    int D = 0;
    int st = check_shape(Q, Q, Q, O, c->B, Nq, c->d_model, c->h, c->variant, &D, "Nq");
    if (st == QMHA_OK) st = check_flag_bits(flags);
    if (st != QMHA_OK) return st;
    if (!lens) return fail(QMHA_ERR_INVALID, "attend_varlen: null lens (a device int32[B])");
    const bool causal = flags & QMHA_FLAG_CAUSAL;
    if (causal && Nq > c->cap)
        return fail(QMHA_ERR_INVALID, "causal attention is bottom-right aligned and needs Nq <= cap (Nq = " + std::to_string(Nq) +
                                          ", cap = " + std::to_string(c->cap) + ")");
    return cache_enqueue(c, &ProfRec::main, stream, "kv_cache attend_varlen launch", kNoLenCheck, [&](const auto& w, int) {
        return qmha::launch_fa_masked(w, Q, O, {c->B, Nq, c->cap, c->h, c->h_kv, c->D, c->d_model, causal, -1, lens},
                                      (hipStream_t)stream);
    });
}

// ---- token-granular lengths: device lengths only, the host `len` is neither read nor changed ----
size_t qmha_kv_cache_tail_bytes(const qmha_kv_cache_t* c) {
    if (!c || c->variant != QMHA_FA_TC_INT8_B) return 0;  // fp16: a row converts on its own
    return qmha::kv_tail_bytes(c->B, c->h_kv, c->D);
}

int qmha_kv_cache_attach_tail(qmha_kv_cache_t* c, void* mem, size_t bytes) {
    if (!c) return fail(QMHA_ERR_INVALID, "null cache");
    const size_t need = qmha_kv_cache_tail_bytes(c);
    if (need == 0) return QMHA_OK;  // nothing to hold
    if (!mem) return fail(QMHA_ERR_INVALID, "attach_tail: null tail memory");
    if (reinterpret_cast<uintptr_t>(mem) % 256 != 0) return fail(QMHA_ERR_INVALID, "attach_tail: tail memory must be 256-byte aligned");
    if (bytes < need)
        return fail(QMHA_ERR_INVALID, "attach_tail: tail memory too small: " + std::to_string(bytes) +
                                          " bytes, qmha_kv_cache_tail_bytes is " + std::to_string(need));
    std::lock_guard<std::mutex> lk(c->mu);
    c->tail = mem;
    return QMHA_OK;
}

int qmha_kv_cache_append_tokens(qmha_kv_cache_t* c, const float* K, const float* V, int n, const int32_t* pos, void* stream) {
    return append_rows({c, "append_tokens", false}, K, V, n, pos, nullptr, stream);
}

int qmha_attend_cached_tokens(qmha_kv_cache_t* c, const float* Q, float* O, int Nq, const int32_t* lens, unsigned flags,
                              void* stream) {
    return attend_rows({c, "attend_tokens", false}, Q, O, Nq, lens, nullptr, flags, stream);
}

// ---- paged caches: a pool of pages and a block table read on the device --------------------
size_t qmha_kv_cache_paged_bytes(int num_pages, int page_rows, int d_model, int h, int h_kv, int variant) {
    if (h < 1 || h_kv < 1 || d_model % h) return 0;
    return qmha_workspace_size(num_pages, page_rows, h_kv * (d_model / h), h_kv, variant);  // the carve of num_pages slices of page_rows rows
}

int qmha_kv_cache_create_paged(qmha_kv_cache_t** out, void* mem, size_t bytes, int B, int num_pages, int page_rows, int max_pages,
                               int d_model, int h, int h_kv, int variant) {
    if (!out) return fail(QMHA_ERR_INVALID, "null cache handle pointer");
    *out = nullptr;
    if (!mem) return fail(QMHA_ERR_INVALID, "null cache memory");
    if (page_rows < 64 || page_rows % 64 != 0)
        return fail(QMHA_ERR_INVALID, "create_paged: page_rows = " + std::to_string(page_rows) +
                                          " must be a positive multiple of 64 (a stage of two 32-row key tiles lies in one page)");
    if (num_pages < 1) return fail(QMHA_ERR_INVALID, "create_paged: num_pages = " + std::to_string(num_pages) + " must be at least 1");
    if (max_pages < 1) return fail(QMHA_ERR_INVALID, "create_paged: max_pages = " + std::to_string(max_pages) + " must be at least 1");
    if ((long long)max_pages * page_rows > (1 << 30))
        return fail(QMHA_ERR_INVALID, "create_paged: the logical capacity max_pages * page_rows exceeds 2^30 rows");
    int D = 0;
    int st = check_shape(mem, mem, mem, mem, B, page_rows, d_model, h, variant, &D, "page_rows");
    if (st == QMHA_OK) st = check_kv_heads(h, h_kv);
    if (st == QMHA_OK) st = not_built(h_kv < h ? kGroupedFeature : "the persistent K/V cache", variant, D);
    if (st != QMHA_OK) return st;
    if (reinterpret_cast<uintptr_t>(mem) % 256 != 0) return fail(QMHA_ERR_INVALID, "cache memory must be 256-byte aligned");
    const size_t need = workspace_bytes(num_pages, page_rows, h_kv, D, variant);
    if (bytes < need)
        return fail(QMHA_ERR_INVALID, "cache memory too small: " + std::to_string(bytes) + " bytes, qmha_kv_cache_paged_bytes is " +
                                          std::to_string(need));
    qmha_kv_cache* c = new qmha_kv_cache;
    c->mem = mem;
    c->B = B, c->cap = max_pages * page_rows, c->d_model = d_model, c->h = h, c->D = D, c->variant = variant;
    c->h_kv = h_kv;
    c->len = 0;
    c->num_pages = num_pages, c->page_rows = page_rows, c->max_pages = max_pages;
    *out = c;
    return QMHA_OK;
}

int qmha_kv_cache_append_paged(qmha_kv_cache_t* c, const float* K, const float* V, int n, const int32_t* pos, const int32_t* table,
                               void* stream) {
    return append_rows({c, "append_paged", true}, K, V, n, pos, table, stream);
}

int qmha_attend_cached_paged(qmha_kv_cache_t* c, const float* Q, float* O, int Nq, const int32_t* lens, const int32_t* table,
                             unsigned flags, void* stream) {
    return attend_rows({c, "attend_paged", true}, Q, O, Nq, lens, table, flags, stream);
}

// ---- a sliding window: the token-granular and the paged attend over the last `window` keys of a row -------
int qmha_attend_cached_tokens_window(qmha_kv_cache_t* c, const float* Q, float* O, int Nq, const int32_t* lens, int window,
                                     unsigned flags, void* stream) {
    return attend_rows({c, "attend_tokens_window", false}, Q, O, Nq, lens, nullptr, flags, stream, &window);
}

int qmha_attend_cached_paged_window(qmha_kv_cache_t* c, const float* Q, float* O, int Nq, const int32_t* lens, const int32_t* table,
                                    int window, unsigned flags, void* stream) {
    return attend_rows({c, "attend_paged_window", true}, Q, O, Nq, lens, table, flags, stream, &window);
}

// ---- split-KV: the token-granular and the paged attend with the key sweep cut into chunks -----------
namespace {

bool split_chunk_ok(const qmha_kv_cache* c, int chunk_rows) { return chunk_rows >= 64 && chunk_rows % 64 == 0 && chunk_rows <= c->cap; }
size_t split_bytes(const qmha_kv_cache* c, int Nq, int chunk_rows) {
    return qmha::split_carve(nullptr, c->B, (c->cap + chunk_rows - 1) / chunk_rows, Nq, c->h, c->D).bytes;
}

// both entry points: `table` null is the contiguous one
int attend_split(qmha_kv_cache_t* c, const char* what, const float* Q, float* O, int Nq, const int32_t* lens, const int32_t* table,
                 bool paged, int chunk_rows, void* scratch, size_t scratch_bytes, unsigned flags, void* stream) {
    const CacheCall k{c, what, paged};
    if (int st = k.operands(Q, O)) return st;
    if (int st = k.attend_words(lens, table, flags)) return st;
    if (int st = k.rows("Nq", Nq)) return st;
    if (!split_chunk_ok(c, chunk_rows))
        return k.bad("chunk_rows = " + std::to_string(chunk_rows) + " must be a multiple of 64 with 64 <= chunk_rows <= cap = " +
                     std::to_string(c->cap) + " (a chunk is a whole number of two-tile stages)");
    if (!scratch) return k.bad("null scratch (qmha_attend_split_bytes bytes of device memory)");
    if (reinterpret_cast<uintptr_t>(scratch) % 256 != 0) return k.bad("scratch must be 256-byte aligned");
    const size_t need = split_bytes(c, Nq, chunk_rows);
    if (scratch_bytes < need)
        return k.bad("scratch too small: " + std::to_string(scratch_bytes) + " bytes, qmha_attend_split_bytes is " + std::to_string(need));
    return cache_enqueue(c, &ProfRec::main, stream, k.label().c_str(), kNoLenCheck, [&](const auto& ws, int) {  // one pair around both launches
        return qmha::launch_fa_split(ws, Q, O, k.attend(Nq, lens, table), chunk_rows, scratch, (hipStream_t)stream);
    });
}

}  // namespace

size_t qmha_attend_split_bytes(const qmha_kv_cache_t* c, int Nq, int chunk_rows) {
    if (!c || Nq < 1 || Nq > c->cap || !split_chunk_ok(c, chunk_rows)) return 0;
    return split_bytes(c, Nq, chunk_rows);
}

int qmha_attend_cached_tokens_split(qmha_kv_cache_t* c, const float* Q, float* O, int Nq, const int32_t* lens, int chunk_rows,
                                    void* scratch, size_t scratch_bytes, unsigned flags, void* stream) {
    return attend_split(c, "attend_tokens_split", Q, O, Nq, lens, nullptr, false, chunk_rows, scratch, scratch_bytes, flags, stream);
}

int qmha_attend_cached_paged_split(qmha_kv_cache_t* c, const float* Q, float* O, int Nq, const int32_t* lens, const int32_t* table,
                                   int chunk_rows, void* scratch, size_t scratch_bytes, unsigned flags, void* stream) {
    return attend_split(c, "attend_paged_split", Q, O, Nq, lens, table, true, chunk_rows, scratch, scratch_bytes, flags, stream);
}

// ---- packed batches: a query / append count per sequence from a device cu[B + 1], no batch axis -----------
namespace {

// both append entry points: `table` null is the contiguous one
int append_packed(qmha_kv_cache_t* c, const char* what, const float* K, const float* V, int total, int max_n, const int32_t* cu,
                  const int32_t* pos, const int32_t* table, bool paged, void* stream) {
    const CacheCall k{c, what, paged};
    if (int st = k.operands(K, V)) return st;
    if (int st = k.words(cu, "cu (a device int32[B + 1])")) return st;
    if (int st = k.words(pos, "pos (a device int32[B])")) return st;
    if (int st = k.table(table)) return st;
    if (int st = k.bound("max_n", total, max_n)) return st;
    return cache_enqueue(
        c, &ProfRec::pre, stream, k.label().c_str(), [&](int) { return k.tail(); },
        [&](const auto& ws, int) {
            return qmha::launch_kv_packed(K, V, ws, static_cast<float*>(c->tail), c->B, total, max_n, c->cap, cu, pos, c->h_kv, c->D,
                                          c->h_kv * c->D, (hipStream_t)stream, c->pages(table));
        });
}

int attend_packed(qmha_kv_cache_t* c, const char* what, const float* Q, float* O, int total, int max_nq, const int32_t* cu,
                  const int32_t* lens, const int32_t* table, bool paged, unsigned flags, void* stream) {
    const CacheCall k{c, what, paged};
    if (int st = k.operands(Q, O)) return st;
    if (int st = k.words(cu, "cu (a device int32[B + 1])")) return st;
    if (int st = k.attend_words(lens, table, flags)) return st;
    if (int st = k.bound("max_nq", total, max_nq)) return st;
    return cache_enqueue(c, &ProfRec::main, stream, k.label().c_str(), kNoLenCheck, [&](const auto& ws, int) {
        return qmha::launch_fa_packed(ws, Q, O, k.attend(max_nq, lens, table), cu, total, (hipStream_t)stream);
    });
}

}  // namespace

int qmha_kv_cache_append_packed(qmha_kv_cache_t* c, const float* K, const float* V, int total, int max_n, const int32_t* cu,
                                const int32_t* pos, void* stream) {
    return append_packed(c, "append_packed", K, V, total, max_n, cu, pos, nullptr, false, stream);
}

int qmha_kv_cache_append_paged_packed(qmha_kv_cache_t* c, const float* K, const float* V, int total, int max_n, const int32_t* cu,
                                      const int32_t* pos, const int32_t* table, void* stream) {
    return append_packed(c, "append_paged_packed", K, V, total, max_n, cu, pos, table, true, stream);
}

int qmha_attend_cached_packed(qmha_kv_cache_t* c, const float* Q, float* O, int total, int max_nq, const int32_t* cu,
                              const int32_t* lens, unsigned flags, void* stream) {
    return attend_packed(c, "attend_packed", Q, O, total, max_nq, cu, lens, nullptr, false, flags, stream);
}

int qmha_attend_cached_paged_packed(qmha_kv_cache_t* c, const float* Q, float* O, int total, int max_nq, const int32_t* cu,
                                    const int32_t* lens, const int32_t* table, unsigned flags, void* stream) {
    return attend_packed(c, "attend_paged_packed", Q, O, total, max_nq, cu, lens, table, true, flags, stream);
}

int qmha_solve_variant(const float* Q, const float* K, const float* V, float* O, int N, int d_model, int h,
                       int variant) {
    // blocking like the reference (launchers.h:64): hipStreamSynchronize.  r04 A/B: polling
    // hipStreamQuery was slower (profiles/r04/ab_sync/summary.txt); r05's spin on a stream-ordered host
    // flag saved ~1 us per call (profiles/r05/ab_solve_sync/) but pinned a host word per thread and a CPU
    // core per waiting thread, so r06 returned to the runtime's synchronisation (round-5 ADVICE)
    int st = qmha_solve_ex(Q, K, V, O, 1, N, d_model, h, variant, nullptr);
    if (st != QMHA_OK) return st;
    QMHA_HIP_TRY(hipStreamSynchronize(nullptr), "solve: hipStreamSynchronize");
    return QMHA_OK;
}

int qmha_quantize_int8(const float* X, int B, int N, int d_model, int h, int8_t* Xi, float* scales, int layout,
                       void* stream) {
    int D = 0;
    int st = check_shape(X, X, X, Xi, B, N, d_model, h, QMHA_FA_TC_INT8_B, &D);
    if (st != QMHA_OK) return st;
    if (!scales || layout < 0 || layout > 2) return fail(QMHA_ERR_INVALID, "bad scales pointer or layout");
    if (layout == 2) {  // per-tensor (head-slice) scales: the per-tensor mode's single-read pass
        const unsigned have = find_variant(QMHA_FA_TC_INT8_PT)->plain;
        if (!built(have, D))
            return fail(QMHA_ERR_NOSYS, "layout 2 (per-tensor scales) is built for d = " + d_list(have) + " only");
        WsLease ws;  // the slice counters; held until the pass is enqueued
        st = lease_workspace(qmha::pt_slice_sync_bytes(B, h), (hipStream_t)stream, &ws);
        if (st != QMHA_OK) return st;
        qmha::Int8Workspace w{};
        w.Ki = Xi;  // the K role: int8 rows
        w.sK = scales;
        w.slice_sync = static_cast<uint32_t*>(ws.ptr);
        QMHA_HIP_TRY(qmha::launch_quant_int8_pt_rows(X, w, B, N, h, D, d_model, (hipStream_t)stream), "quant_int8_pt launch");
        return QMHA_OK;
    }
    // The pre-pass kernel with X in one role only: the Q role (row layout) or the V role (the
    // V^T operand order); nothing else is written, no workspace is needed.
    qmha::Int8Workspace w{};
    void* vout = nullptr;
    int v_mode = 1, role = 0;
    if (layout == 0) {
        w.Qi = Xi;
        w.sQ = scales;
    } else {
        vout = Xi;
        v_mode = 0;
        w.sV = scales;
        role = 2;
    }
    QMHA_HIP_TRY(qmha::launch_quant_int8(X, X, X, w, vout, v_mode, B, N, h, D, d_model, (hipStream_t)stream, role, 1),
                 "quant_int8 launch");
    return QMHA_OK;
}

int qmha_debug_qk_int32(const float* Q, const float* K, int N, int d_model, int h, int head, int32_t* S) {
    int D = 0;
    int st = check_shape(Q, K, Q, S, 1, N, d_model, h, QMHA_FA_TC_INT8_B, &D);
    if (st != QMHA_OK) return st;
    if (head < 0 || head >= h) return fail(QMHA_ERR_INVALID, "head out of range");
    return debug_run(qmha::int8_workspace_bytes(1, N, h, D, /*with_q=*/true), [&](void* ws) -> int {
        const qmha::Int8Workspace w = qmha::int8_carve(ws, 1, N, h, D, /*with_q=*/true);
        QMHA_HIP_TRY(qmha::launch_quant_int8(Q, K, Q, w, w.Vh, 1, 1, N, h, D, d_model, nullptr), "quant_int8 launch");
        QMHA_HIP_TRY(qmha::launch_debug_qk_int32(w, N, D, head, S, nullptr), "debug_qk launch");
        return QMHA_OK;
    });
}

int qmha_debug_fa_int8_dump(const float* Q, const float* K, const float* V, float* O, int B, int N, int d_model,
                            int h, int32_t* S, int8_t* Qi, float* sQ) {
    int D = 0;
    int st = check_shape(Q, K, V, O, B, N, d_model, h, QMHA_FA_TC_INT8_B, &D);
    if (st != QMHA_OK) return st;
    if (!S || !Qi || !sQ || ((D == 32 || D == 64 || D == 128) && N < 64))
        return fail(QMHA_ERR_INVALID,
                    "debug dump: needs S/Qi/sQ buffers and, at d = 32 / 64 / 128, N >= 64 (the pipelined kernel)");
    return debug_run(qmha::int8_workspace_bytes(B, N, h, D), [&](void* ws) -> int {
        const qmha::Int8Workspace w = qmha::int8_carve(ws, B, N, h, D);
        QMHA_HIP_TRY(qmha::launch_quant_int8(Q, K, V, w, w.Vh, /*v_mode=*/1, B, N, h, D, d_model, nullptr, /*first_tensor=*/1),
                     "quant_int8 launch");
        QMHA_HIP_TRY(qmha::launch_fa_int8_dump(w, Q, O, B, N, h, D, d_model, qmha::QkDump{S, Qi, sQ}, nullptr),
                     "fa_int8 dump launch");
        return QMHA_OK;
    });
}

int qmha_debug_fa_int8_pstage(const float* Q, const float* K, const float* V, float* O, int B, int Nq, int Nk, int d_model,
                              int h, unsigned flags, int32_t* S, int8_t* Qi, float* sQ, float* m, float* sP, int8_t* Pi,
                              int32_t* T, float* l) {
    // qmha_solve_rect's checks for fa_tc_int8_b, then run()'s choice of main kernel
    int D = 0;
    const int st = check_call({Q, K, V, O, B, Nq, Nk, d_model, h, h, QMHA_FA_TC_INT8_B, flags, false, false, nullptr, 0}, &D);
    if (st != QMHA_OK) return st;
    const bool causal = flags & QMHA_FLAG_CAUSAL;
    if (!S || !Qi || !sQ || !m || !sP || !Pi || !T || !l) return fail(QMHA_ERR_INVALID, "debug P-stage dump: null buffer");
    return debug_run(qmha::int8_workspace_bytes(B, Nk, h, D), [&](void* ws) -> int {
        const qmha::Int8Workspace w = qmha::int8_carve(ws, B, Nk, h, D);
        QMHA_HIP_TRY(qmha::launch_quant_int8(Q, K, V, w, w.Vh, /*v_mode=*/1, B, Nk, h, D, d_model, nullptr, /*first_tensor=*/1),
                     "quant_int8 launch");
        const qmha::QkDump dbg{S, Qi, sQ};
        const qmha::PDump pd{m, sP, Pi, T, l};
        if (causal || Nq != Nk)
            QMHA_HIP_TRY(qmha::launch_fa_int8_masked_pstage_dump(w, Q, O, {B, Nq, Nk, h, h, D, d_model, causal, -1, nullptr}, dbg, pd),
                         "fa_int8 masked P-stage dump launch");
        else
            QMHA_HIP_TRY(qmha::launch_fa_int8_pstage_dump(w, Q, O, B, Nk, h, D, d_model, dbg, pd), "fa_int8 P-stage dump launch");
        return QMHA_OK;
    });
}

int qmha_debug_fa_int8_pt_dump(const float* Q, const float* K, const float* V, float* O, int B, int N, int d_model,
                               int h, int32_t* S, int8_t* Qi, float* sQ) {
    int D = 0;
    int st = check_shape(Q, K, V, O, B, N, d_model, h, QMHA_FA_TC_INT8_PT, &D);
    if (st != QMHA_OK) return st;
    if (!S || !Qi || !sQ) return fail(QMHA_ERR_INVALID, "debug dump: needs S/Qi/sQ buffers");
    return debug_run(qmha::int8_pt_workspace_bytes(B, N, h, D), [&](void* ws) -> int {
        const qmha::Int8Workspace w = qmha::int8_pt_carve(ws, B, N, h, D);
        QMHA_HIP_TRY(qmha::launch_quant_int8_pt(Q, K, V, w, B, N, h, D, d_model, nullptr), "quant_int8_pt launch");
        QMHA_HIP_TRY(qmha::launch_fa_int8_pt_dump(w, Q, O, B, N, h, D, d_model, qmha::QkDump{S, Qi, sQ}, nullptr),
                     "fa_int8_pt dump launch");
        return QMHA_OK;
    });
}

int qmha_variant_from_name(const char* name) {
    if (!name) return -1;
    for (const VariantRow& r : kVariants)
        if (!std::strcmp(name, r.name)) return r.id;
    return -1;
}

const char* qmha_variant_name(int v) {
    const VariantRow* r = find_variant(v);
    return r ? r->name : "unknown";
}

const char* qmha_status_string(int s) {
    switch (s) {
        case QMHA_OK: return "ok";
        case QMHA_ERR_INVALID: return "invalid argument";
        case QMHA_ERR_HIP: return "HIP error";
        case QMHA_ERR_NOMEM: return "out of device memory";
        case QMHA_ERR_NOSYS: return "not supported";
        default: return "unknown status";
    }
}

const char* qmha_version(void) { return QMHA_VERSION_STRING; }

const char* qmha_last_error(void) { return g_last_error.c_str(); }

int64_t qmha_debug_set_pt_wait(int64_t ticks) { return qmha::set_pt_wait_ticks(ticks); }

int qmha_set_overlap_chunks(int n) {
    const int prev = overlap_chunks(1 << 30);
    g_overlap_chunks.store(clamp_chunks(n));
    return prev;
}

void qmha_profile_enable(int on) {
    std::lock_guard<std::mutex> lk(g_prof_mu);
    g_prof_on = on != 0;
}

int qmha_profile_collect(double* main_ms, long long* launches, double* prepass_ms) {
    std::vector<ProfRec> recs;
    {
        std::lock_guard<std::mutex> lk(g_prof_mu);
        recs.swap(g_prof_recs);
    }
    double tm = 0.0, tp = 0.0;
    for (auto& r : recs) {
        for (auto* v : {&r.main, &r.pre}) {
            for (auto& pr : *v) {
                QMHA_HIP_TRY(hipEventSynchronize(pr.second), "hipEventSynchronize");
                float a = 0.0f;
                QMHA_HIP_TRY(hipEventElapsedTime(&a, pr.first, pr.second), "hipEventElapsedTime");
                (v == &r.main ? tm : tp) += a;
            }
        }
    }
    {
        std::lock_guard<std::mutex> lk(g_prof_mu);
        for (auto& r : recs)
            for (auto* v : {&r.main, &r.pre})
                for (auto& pr : *v) {
                    g_event_pool.push_back(pr.first);
                    g_event_pool.push_back(pr.second);
                }
    }
    if (main_ms) *main_ms = tm;
    if (prepass_ms) *prepass_ms = tp;
    if (launches) *launches = (long long)recs.size();
    return QMHA_OK;
}

void qmha_release_workspaces(void) {
    // each slot under its lease: a call still enqueueing on it finishes first; buffers, side stream and
    // events go after the device has drained (work on any stream may still use them)
    std::lock_guard<std::mutex> lk(g_ws_mu);
    for (auto& kv : g_ws) {
        WsSlot& s = *kv.second;
        std::lock_guard<std::mutex> lease(s.lease);
        (void)hipDeviceSynchronize();
        reap_retired(s, true);
        if (s.ptr) (void)hipFree(s.ptr);
        s.ptr = nullptr;
        s.bytes = 0;
        if (s.side) (void)hipStreamSynchronize(s.side);  // a slot of another device than the current one
        for (hipEvent_t e : s.ready) (void)hipEventDestroy(e);
        s.ready.clear();
        if (s.start) (void)hipEventDestroy(s.start);
        if (s.side) (void)hipStreamDestroy(s.side);
        s.start = nullptr;
        s.side = nullptr;
    }
}

#ifndef QMHA_NO_DEFAULT_SOLVE
// libqmha.so's `solve` = the north-star drop-in target, fa_tc_int8_b.
void solve(const float* Q, const float* K, const float* V, float* output, int N, int d_model, int h) {
    int st = qmha_solve_variant(Q, K, V, output, N, d_model, h, QMHA_FA_TC_INT8_B);
    if (st != QMHA_OK) std::fprintf(stderr, "qmha solve(fa_tc_int8_b): %s: %s\n", qmha_status_string(st), qmha_last_error());
}
#endif

}  // extern "C"
