// Compiled PyTorch extension `torch_ext` -- the drop-in for the reference's pybind module
// (extensions/torch/torch_ext.cpp:11-58, built per kernel by extensions/torch/setup.py:21-43).
// Same module name, function name, argument names/defaults and TORCH_CHECK messages, so
// `import torch_ext; torch_ext.flash_solve(Q, K, V, d_model, num_heads)` works unchanged.
// It is a thin shim over the C-ABI in libqmha.so (include/launchers.h): no kernel code here.
//
// Differences from the reference, all additive (same as quantizedmha_amd/torch_ext.py):
//   * `kernel` really selects the variant (the reference warns and runs its build-time kernel;
//     an unknown name still warns and routes to fa_tc_int8_b, torch_ext.cpp:32-34);
//   * a 3-D [B, N, d_model] input is B sequences in one launch;
//   * the work is enqueued on PyTorch's current HIP stream (ordered with the caller's other
//     ops) instead of private streams plus a blocking device synchronisation;
//   * `causal` (trailing, default false): causal attention through qmha_solve_opts;
//   * `flash_solve_rect` (a second function, same arguments): K and V of one shape, Q with its own row count,
//     through qmha_solve_rect; `flash_solve` itself still wants one shape;
//   * `KVCache` (a class): a persistent quantised K/V cache through qmha_kv_cache_* / qmha_attend_cached;
//   * `flash_solve_gqa` and `GroupedKVCache`: the two above with `num_kv_heads` K/V heads shared by the query heads
//     (grouped-query attention, qmha_solve_gqa / qmha_kv_cache_create_gqa); None is the multi-head form;
//   * both caches' `append_at` / `attend_varlen`: a row / a length per sequence in int32 [B] device tensors that the
//     kernels read (qmha_kv_cache_append_at / qmha_attend_cached_varlen);
//   * both caches' `enable_tokens` / `append_tokens` / `attend_tokens`: the same at any length -- any number of rows at any
//     row, any Nq, causal (qmha_kv_cache_attach_tail / qmha_kv_cache_append_tokens / qmha_attend_cached_tokens);
//   * `PagedKVCache`: a pool of pages and a caller-owned block table on the device, `append_paged` / `attend_paged`
//     (qmha_kv_cache_create_paged / qmha_kv_cache_append_paged / qmha_attend_cached_paged);
//   * all three caches' `enable_split` / `attend_tokens_split` (`attend_paged_split`) / `split_partials`: the attend with
//     the key sweep in chunks over a scratch the object owns (qmha_attend_cached_tokens_split / _paged_split);
//   * all three caches' `append_packed` / `attend_packed` (`append_paged_packed` / `attend_paged_packed`): a count per
//     sequence from a device cu[B + 1] over operands without a batch axis (qmha_kv_cache_append_packed / ..._paged_packed);
//   * all three caches' `attend_tokens_window` (`attend_paged_window`): the attend over the last `window` keys of a row
//     (qmha_attend_cached_tokens_window / _paged_window);
//   * a rejected shape raises (TORCH_CHECK on the C-ABI status) instead of a device assert.
#include <torch/extension.h>
// ROCm PyTorch reports HIP devices as device type "cuda": the guard / current-stream
// accessors for such tensors are the "MasqueradingAsCUDA" ones
#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>

#include <climits>
#include <optional>
#include <string>
#include <tuple>

#include "launchers.h"

using torch::Tensor;

// Q, K and V of a solve, made contiguous: all on the GPU and float32, with the reference's messages
struct Inputs { Tensor Q, K, V; };
static Inputs fp32_inputs(const Tensor& Q, const Tensor& K, const Tensor& V, int64_t d_model) {
    TORCH_CHECK(Q.is_cuda() && K.is_cuda() && V.is_cuda(), "Inputs must be CUDA tensors");
    TORCH_CHECK(Q.dtype() == torch::kFloat32, "Q must be float32");
    TORCH_CHECK(K.dtype() == torch::kFloat32, "K must be float32");
    TORCH_CHECK(V.dtype() == torch::kFloat32, "V must be float32");
    Inputs in{Q.contiguous(), K.contiguous(), V.contiguous()};
    TORCH_CHECK(d_model > 0 && in.Q.numel() % d_model == 0, "Q.numel() must be divisible by d_model");
    return in;
}

// an unknown kernel name warns and routes to the default (torch_ext.cpp:32-34)
static int known_variant(const std::string& kernel) {
    const int variant = qmha_variant_from_name(kernel.c_str());
    if (variant >= 0) return variant;
    TORCH_WARN("Kernel selection supports fa, fa_tc_v1a, fa_tc_int8_b, unfused, fa_mfma, fa_tc_int8_pt; '", kernel,
               "' routing to default 'fa_tc_int8_b'");
    return QMHA_FA_TC_INT8_B;
}

// the caller's `out`, checked against Qc by size, or a new tensor like Qc
static Tensor out_for(const std::optional<Tensor>& out, const Tensor& Qc) {
    if (!out) return torch::empty_like(Qc);
    TORCH_CHECK(out->numel() == Qc.numel() && out->dtype() == torch::kFloat32 && out->device() == Qc.device() &&
                    out->is_contiguous(),
                "out must be a contiguous float32 tensor of Q's size on Q's device");
    return *out;
}

// [B, N, width] is B sequences; anything else one sequence of numel / width rows (reference torch_ext.cpp:23-25)
static int64_t rows_of(const Tensor& t, int64_t width, int64_t* B) {
    const bool batched = t.dim() == 3 && t.size(2) == width;
    *B = batched ? t.size(0) : 1;
    return batched ? t.size(1) : t.numel() / width;
}

// `device` made current for as long as the result lives, and PyTorch's current stream there
struct OnStream {
    c10::hip::HIPGuardMasqueradingAsCUDA guard;
    hipStream_t stream;
};
static OnStream current_stream(const c10::Device& device) {
    return {c10::hip::HIPGuardMasqueradingAsCUDA(device), c10::hip::getCurrentHIPStreamMasqueradingAsCUDA(device.index()).stream()};
}

static Tensor flash_solve(const Tensor& Q, const Tensor& K, const Tensor& V, int64_t d_model, int64_t num_heads,
                          const std::string& kernel = "fa_tc_int8_b", bool causal = false) {
    const Inputs in = fp32_inputs(Q, K, V, d_model);
    TORCH_CHECK(in.K.sizes() == in.Q.sizes() && in.V.sizes() == in.Q.sizes(), "Q, K and V must have the same shape");
    int64_t B = 1;
    const int64_t N = rows_of(in.Q, d_model, &B);
    const int variant = known_variant(kernel);
    auto out = torch::empty_like(in.Q);
    const OnStream on = current_stream(in.Q.device());
    // causal = false enqueues exactly what qmha_solve_ex does (flags == 0)
    const int st = qmha_solve_opts(in.Q.data_ptr<float>(), in.K.data_ptr<float>(), in.V.data_ptr<float>(),
                                   out.data_ptr<float>(), static_cast<int>(B), static_cast<int>(N),
                                   static_cast<int>(d_model), static_cast<int>(num_heads), variant,
                                   causal ? QMHA_FLAG_CAUSAL : 0u, nullptr, 0, on.stream);
    TORCH_CHECK(st == QMHA_OK, "flash_solve", "(", kernel, "): ", qmha_status_string(st), ": ", qmha_last_error());
    return out;
}

// flash_solve with a query length of its own (qmha_solve_rect): K and V share one shape, Q has its own row
// count and the same batch count; the result is shaped like Q.  causal: bottom-right aligned.
// num_kv_heads (flash_solve_gqa): K and V are [Nk, num_kv_heads * d] or [B, Nk, num_kv_heads * d]; none: flash_solve_rect
static Tensor solve_rect(const Tensor& Q, const Tensor& K, const Tensor& V, int64_t d_model, int64_t num_heads,
                         std::optional<int64_t> num_kv_heads, const std::string& kernel, bool causal, const char* what) {
    const Inputs in = fp32_inputs(Q, K, V, d_model);
    TORCH_CHECK(in.K.sizes() == in.V.sizes(), "K and V must have the same shape");
    int64_t kv_model = d_model;
    if (num_kv_heads) {
        TORCH_CHECK(num_heads >= 1 && d_model % num_heads == 0 && *num_kv_heads >= 1,
                    "d_model must be divisible by num_heads, and num_kv_heads positive");
        kv_model = *num_kv_heads * (d_model / num_heads);
    }
    TORCH_CHECK(in.K.numel() % kv_model == 0,
                num_kv_heads ? "K.numel() must be divisible by num_kv_heads * d" : "K.numel() must be divisible by d_model");
    int64_t B = 1, Bk = 1;
    const int64_t Nq = rows_of(in.Q, d_model, &B), Nk = rows_of(in.K, kv_model, &Bk);
    TORCH_CHECK(B == Bk, "Q and K must have the same batch count");
    const int variant = known_variant(kernel);
    auto out = torch::empty_like(in.Q);
    const OnStream on = current_stream(in.Q.device());
    const unsigned flags = causal ? QMHA_FLAG_CAUSAL : 0u;
    const int st =
        num_kv_heads
            ? qmha_solve_gqa(in.Q.data_ptr<float>(), in.K.data_ptr<float>(), in.V.data_ptr<float>(), out.data_ptr<float>(),
                             static_cast<int>(B), static_cast<int>(Nq), static_cast<int>(Nk), static_cast<int>(d_model),
                             static_cast<int>(num_heads), static_cast<int>(*num_kv_heads), variant, flags, nullptr, 0, on.stream)
            : qmha_solve_rect(in.Q.data_ptr<float>(), in.K.data_ptr<float>(), in.V.data_ptr<float>(), out.data_ptr<float>(),
                              static_cast<int>(B), static_cast<int>(Nq), static_cast<int>(Nk), static_cast<int>(d_model),
                              static_cast<int>(num_heads), variant, flags, nullptr, 0, on.stream);
    TORCH_CHECK(st == QMHA_OK, what, "(", kernel, "): ", qmha_status_string(st), ": ", qmha_last_error());
    return out;
}

static Tensor flash_solve_rect(const Tensor& Q, const Tensor& K, const Tensor& V, int64_t d_model, int64_t num_heads,
                               const std::string& kernel = "fa_tc_int8_b", bool causal = false) {
    return solve_rect(Q, K, V, d_model, num_heads, std::nullopt, kernel, causal, "flash_solve_rect");
}

// flash_solve_rect for grouped-query attention (qmha_solve_gqa); num_kv_heads = None is flash_solve_rect
static Tensor flash_solve_gqa(const Tensor& Q, const Tensor& K, const Tensor& V, int64_t d_model, int64_t num_heads,
                              std::optional<int64_t> num_kv_heads, const std::string& kernel = "fa_tc_int8_b",
                              bool causal = false) {
    return solve_rect(Q, K, V, d_model, num_heads, num_kv_heads, kernel, causal, "flash_solve_gqa");
}

// What the cache classes ask of their tensors.
// a per-sequence int32 [B] tensor on the cache's device, contiguous: the kernel reads it, the host does not
static void cache_per_seq(const Tensor& t, const char* name, int64_t B, const c10::Device& device) {
    TORCH_CHECK(t.is_cuda(), name, " must be a CUDA tensor");
    TORCH_CHECK(t.dtype() == torch::kInt32, name, " must be int32");
    TORCH_CHECK(t.device() == device, name, " must be on the cache's device");
    TORCH_CHECK(t.dim() == 1 && t.size(0) == B && t.is_contiguous(), name, " must be a contiguous tensor of shape [B = ", B, "]");
}
// [B, n, d_model] fp32 on the cache's device, contiguous; [n, d_model] for B = 1
static Tensor cache_rows(const Tensor& X, const char* name, int64_t width, int64_t B, const c10::Device& device) {
    TORCH_CHECK(X.is_cuda(), "Inputs must be CUDA tensors");
    TORCH_CHECK(X.dtype() == torch::kFloat32, name, " must be float32");
    TORCH_CHECK(X.device() == device, name, " must be on the cache's device");
    auto Xc = X.contiguous();
    if (Xc.dim() == 2 && B == 1) Xc = Xc.unsqueeze(0);
    TORCH_CHECK(Xc.dim() == 3 && Xc.size(0) == B && Xc.size(2) == width, name, " must be [B = ", B, ", n, d_model = ", width, "]",
                B == 1 ? " or [n, d_model]" : "");
    return Xc;
}

// A packed operand: fp32 [total, width] on the cache's device, contiguous, no batch axis
static Tensor cache_packed_rows(const Tensor& X, const char* name, int64_t width, const c10::Device& device) {
    TORCH_CHECK(X.is_cuda(), "Inputs must be CUDA tensors");
    TORCH_CHECK(X.dtype() == torch::kFloat32, name, " must be float32");
    TORCH_CHECK(X.device() == device, name, " must be on the cache's device");
    auto Xc = X.contiguous();
    TORCH_CHECK(Xc.dim() == 2 && Xc.size(0) >= 1 && Xc.size(1) == width, name, " must be [total, d_model = ", width,
                "] (packed: no batch axis)");
    return Xc;
}
// cu: int32 [B + 1] on the cache's device, contiguous: the kernel reads it, the host does not
static void cache_cu(const Tensor& t, int64_t B, const c10::Device& device) {
    TORCH_CHECK(t.is_cuda(), "cu must be a CUDA tensor");
    TORCH_CHECK(t.dtype() == torch::kInt32, "cu must be int32");
    TORCH_CHECK(t.device() == device, "cu must be on the cache's device");
    TORCH_CHECK(t.dim() == 1 && t.size(0) == B + 1 && t.is_contiguous(), "cu must be a contiguous tensor of shape [B + 1 = ", B + 1, "]");
}
// O of a packed attend: the caller's, of Q's shape, or zeros (rows outside every range are not written by the call)
static Tensor packed_out(const std::optional<Tensor>& out_opt, const Tensor& Qc) {
    if (!out_opt) return torch::zeros_like(Qc);
    const Tensor& out = *out_opt;
    TORCH_CHECK(out.is_cuda() && out.dtype() == torch::kFloat32 && out.device() == Qc.device() && out.is_contiguous() &&
                    out.sizes() == Qc.sizes(),
                "out must be a contiguous float32 CUDA tensor of Q's shape on Q's device");
    return out;
}

// The split-KV scratch of a cache (enable_split; include/launchers.h has the layout): what both cache classes keep for
// attend_tokens_split / attend_paged_split, and the views split_partials hands out.
struct SplitState {
    int64_t chunk_rows = 0, max_nq = 0;
    Tensor scratch;

    void enable(qmha_kv_cache_t* handle, int64_t chunk, int64_t nq, int64_t cap, const c10::Device& device) {
        const size_t bytes = qmha_attend_split_bytes(handle, static_cast<int>(nq), static_cast<int>(chunk));
        TORCH_CHECK(bytes > 0, "enable_split: chunk_rows = ", chunk, " must be a multiple of 64 with 64 <= chunk_rows <= cap = ", cap,
                    ", and 1 <= max_nq = ", nq, " <= cap");
        chunk_rows = chunk, max_nq = nq;
        scratch = torch::zeros({static_cast<int64_t>(bytes)}, torch::TensorOptions().dtype(torch::kUInt8).device(device));
    }
    void ready(int64_t Nq, const char* what) const {
        TORCH_CHECK(scratch.defined(), what, ": call enable_split(chunk_rows) first");
        TORCH_CHECK(Nq <= max_nq, what, ": Nq = ", Nq, " rows exceed enable_split's max_nq = ", max_nq);
    }
    // (Oc [B, NC, Nq, d_model], m [B, NC, Nq, heads], l [B, NC, Nq, heads]) of the last split attend of Nq rows
    std::tuple<Tensor, Tensor, Tensor> partials(qmha_kv_cache_t* handle, int64_t Nq, int64_t B, int64_t cap, int64_t d_model,
                                                int64_t heads) const {
        ready(Nq, "split_partials");
        TORCH_CHECK(Nq >= 1, "split_partials: Nq must be at least 1");
        const int64_t nc = (cap + chunk_rows - 1) / chunk_rows, rows = B * nc * Nq;
        const auto al = [](int64_t x) { return (x + 255) / 256 * 256; };  // each array starts on a multiple of 256 bytes
        const int64_t o_bytes = 4 * rows * d_model, s_bytes = 4 * rows * heads;
        TORCH_CHECK(static_cast<size_t>(al(o_bytes) + 2 * al(s_bytes)) ==
                        qmha_attend_split_bytes(handle, static_cast<int>(Nq), static_cast<int>(chunk_rows)),
                    "split_partials: the scratch layout is not the library's");
        const auto arr = [&](int64_t off, int64_t bytes, int64_t width) {
            return scratch.slice(0, off, off + bytes).view(torch::kFloat32).view({B, nc, Nq, width});
        };
        return {arr(0, o_bytes, d_model), arr(al(o_bytes), s_bytes, heads), arr(al(o_bytes) + al(s_bytes), s_bytes, heads)};
    }
    std::optional<Tensor> tensor() const { return scratch.defined() ? std::optional<Tensor>(scratch) : std::nullopt; }
};

// A persistent quantised K/V cache (qmha_kv_cache_*): the compiled form of quantizedmha_amd/torch_ext.py's KVCache.
// Owns a uint8 tensor of qmha_kv_cache_bytes and the host handle; append / attend run on PyTorch's current stream.
class KVCache {
public:
    // num_kv_heads (GroupedKVCache): the cache holds that many K/V heads, shared by the num_heads query heads
    KVCache(int64_t B, int64_t cap, int64_t d_model, int64_t num_heads, const std::string& kernel, const std::string& device,
            std::optional<int64_t> num_kv_heads = std::nullopt)
        : B_(B), cap_(cap), d_model_(d_model), kv_model_(d_model), num_heads_(num_heads), kernel_(kernel) {
        const int variant = qmha_variant_from_name(kernel.c_str());
        TORCH_CHECK(variant >= 0, "KVCache: unknown kernel '", kernel, "'");
        c10::Device dev(device);
        TORCH_CHECK(dev.is_cuda(), "KVCache needs a CUDA device");
        // grouped: the row width of K and V (a bad head count is left to the library's checks) and the carve of h_kv heads
        if (num_kv_heads && num_heads > 0 && d_model % num_heads == 0) kv_model_ = *num_kv_heads * (d_model / num_heads);
        const size_t bytes =
            num_kv_heads ? (*num_kv_heads > 0 ? qmha_kv_cache_bytes(static_cast<int>(B), static_cast<int>(cap),
                                                                    static_cast<int>(kv_model_), static_cast<int>(*num_kv_heads), variant)
                                              : 0)
                         : qmha_kv_cache_bytes(static_cast<int>(B), static_cast<int>(cap), static_cast<int>(d_model),
                                               static_cast<int>(num_heads), variant);
        mem_ = torch::zeros({static_cast<int64_t>(bytes > 0 ? bytes : 1)}, torch::TensorOptions().dtype(torch::kUInt8).device(dev));
        const int st =
            num_kv_heads
                ? qmha_kv_cache_create_gqa(&handle_, mem_.data_ptr(), bytes, static_cast<int>(B), static_cast<int>(cap),
                                           static_cast<int>(d_model), static_cast<int>(num_heads), static_cast<int>(*num_kv_heads), variant)
                : qmha_kv_cache_create(&handle_, mem_.data_ptr(), bytes, static_cast<int>(B), static_cast<int>(cap),
                                       static_cast<int>(d_model), static_cast<int>(num_heads), variant);
        TORCH_CHECK(st == QMHA_OK, "KVCache", "(", kernel, "): ", qmha_status_string(st), ": ", qmha_last_error());
    }
    ~KVCache() { qmha_kv_cache_destroy(handle_); }
    KVCache(const KVCache&) = delete;
    KVCache& operator=(const KVCache&) = delete;

    int64_t len() const { return qmha_kv_cache_len(handle_); }
    int64_t cap() const { return cap_; }
    Tensor mem() const { return mem_; }

    void append(const Tensor& K, const Tensor& V) {
        auto Kc = rows(K, "K", kv_model_), Vc = rows(V, "V", kv_model_);
        TORCH_CHECK(Kc.sizes() == Vc.sizes(), "K and V must have the same shape");
        const OnStream on = current_stream(mem_.device());
        const int st = qmha_kv_cache_append(handle_, Kc.data_ptr<float>(), Vc.data_ptr<float>(), static_cast<int>(Kc.size(1)), on.stream);
        TORCH_CHECK(st == QMHA_OK, "KVCache.append", "(", kernel_, "): ", qmha_status_string(st), ": ", qmha_last_error());
    }

    Tensor attend(const Tensor& Q, bool causal) {
        auto Qc = rows(Q, "Q", d_model_);
        auto out = torch::empty_like(Qc);
        const OnStream on = current_stream(mem_.device());
        const int st = qmha_attend_cached(handle_, Qc.data_ptr<float>(), out.data_ptr<float>(), static_cast<int>(Qc.size(1)),
                                          causal ? QMHA_FLAG_CAUSAL : 0u, on.stream);
        TORCH_CHECK(st == QMHA_OK, "KVCache.attend", "(", kernel_, "): ", qmha_status_string(st), ": ", qmha_last_error());
        return out.view(Q.sizes());
    }

    void truncate(int64_t n) {
        const int st = qmha_kv_cache_truncate(handle_, static_cast<int>(n));
        TORCH_CHECK(st == QMHA_OK, "KVCache.truncate: ", qmha_status_string(st), ": ", qmha_last_error());
    }

    // append with a row per sequence (qmha_kv_cache_append_at): pos is int32 [B] on the device, read by the kernel
    void append_at(const Tensor& K, const Tensor& V, const Tensor& pos) {
        auto Kc = rows(K, "K", kv_model_), Vc = rows(V, "V", kv_model_);
        TORCH_CHECK(Kc.sizes() == Vc.sizes(), "K and V must have the same shape");
        per_seq(pos, "pos");
        const OnStream on = current_stream(mem_.device());
        const int st = qmha_kv_cache_append_at(handle_, Kc.data_ptr<float>(), Vc.data_ptr<float>(), static_cast<int>(Kc.size(1)),
                                               pos.data_ptr<int32_t>(), on.stream);
        TORCH_CHECK(st == QMHA_OK, "KVCache.append_at", "(", kernel_, "): ", qmha_status_string(st), ": ", qmha_last_error());
    }

    // attend with a length per sequence (qmha_attend_cached_varlen): lens is int32 [B] on the device, read by the kernel
    Tensor attend_varlen(const Tensor& Q, const Tensor& lens, bool causal, std::optional<Tensor> out_opt) {
        auto Qc = rows(Q, "Q", d_model_);
        per_seq(lens, "lens");
        Tensor out = out_for(out_opt, Qc);
        const OnStream on = current_stream(mem_.device());
        const int st = qmha_attend_cached_varlen(handle_, Qc.data_ptr<float>(), out.data_ptr<float>(), static_cast<int>(Qc.size(1)),
                                                 lens.data_ptr<int32_t>(), causal ? QMHA_FLAG_CAUSAL : 0u, on.stream);
        TORCH_CHECK(st == QMHA_OK, "KVCache.attend_varlen", "(", kernel_, "): ", qmha_status_string(st), ": ", qmha_last_error());
        return out_opt ? out : out.view(Q.sizes());
    }

    // allocate and attach the tail of raw rows append_tokens needs (qmha_kv_cache_attach_tail); once, outside a capture
    void enable_tokens() {
        if (tail_.defined()) return;
        const size_t bytes = qmha_kv_cache_tail_bytes(handle_);
        tail_ = torch::zeros({static_cast<int64_t>(bytes > 0 ? bytes : 1)}, torch::TensorOptions().dtype(torch::kUInt8).device(mem_.device()));
        const int st = qmha_kv_cache_attach_tail(handle_, tail_.data_ptr(), bytes);
        TORCH_CHECK(st == QMHA_OK, "KVCache.enable_tokens", "(", kernel_, "): ", qmha_status_string(st), ": ", qmha_last_error());
    }
    std::optional<Tensor> tail() const { return tail_.defined() ? std::optional<Tensor>(tail_) : std::nullopt; }

    // append_at for any number of rows at any row (qmha_kv_cache_append_tokens)
    void append_tokens(const Tensor& K, const Tensor& V, const Tensor& pos) {
        auto Kc = rows(K, "K", kv_model_), Vc = rows(V, "V", kv_model_);
        TORCH_CHECK(Kc.sizes() == Vc.sizes(), "K and V must have the same shape");
        per_seq(pos, "pos");
        const OnStream on = current_stream(mem_.device());
        const int st = qmha_kv_cache_append_tokens(handle_, Kc.data_ptr<float>(), Vc.data_ptr<float>(), static_cast<int>(Kc.size(1)),
                                                   pos.data_ptr<int32_t>(), on.stream);
        TORCH_CHECK(st == QMHA_OK, "KVCache.append_tokens", "(", kernel_, "): ", qmha_status_string(st), ": ", qmha_last_error());
    }

    // causal attend_varlen for any Nq and any lengths (qmha_attend_cached_tokens)
    Tensor attend_tokens(const Tensor& Q, const Tensor& lens, std::optional<Tensor> out_opt) {
        auto Qc = rows(Q, "Q", d_model_);
        per_seq(lens, "lens");
        Tensor out = out_for(out_opt, Qc);
        const OnStream on = current_stream(mem_.device());
        const int st = qmha_attend_cached_tokens(handle_, Qc.data_ptr<float>(), out.data_ptr<float>(), static_cast<int>(Qc.size(1)),
                                                 lens.data_ptr<int32_t>(), QMHA_FLAG_CAUSAL, on.stream);
        TORCH_CHECK(st == QMHA_OK, "KVCache.attend_tokens", "(", kernel_, "): ", qmha_status_string(st), ": ", qmha_last_error());
        return out_opt ? out : out.view(Q.sizes());
    }

    // attend_tokens over the last `window` keys of a row (qmha_attend_cached_tokens_window)
    Tensor attend_tokens_window(const Tensor& Q, const Tensor& lens, int64_t window, std::optional<Tensor> out_opt) {
        auto Qc = rows(Q, "Q", d_model_);
        per_seq(lens, "lens");
        TORCH_CHECK(window >= INT_MIN && window <= INT_MAX, "attend_tokens_window: window = ", window, " does not fit an int");
        Tensor out = out_for(out_opt, Qc);
        const OnStream on = current_stream(mem_.device());
        const int st = qmha_attend_cached_tokens_window(handle_, Qc.data_ptr<float>(), out.data_ptr<float>(), static_cast<int>(Qc.size(1)),
                                                        lens.data_ptr<int32_t>(), static_cast<int>(window), QMHA_FLAG_CAUSAL, on.stream);
        TORCH_CHECK(st == QMHA_OK, "KVCache.attend_tokens_window", "(", kernel_, "): ", qmha_status_string(st), ": ", qmha_last_error());
        return out_opt ? out : out.view(Q.sizes());
    }

    // allocate the scratch of the split-KV attend (qmha_attend_split_bytes at Nq = max_nq); once, outside a capture
    void enable_split(int64_t chunk_rows, int64_t max_nq) { split_.enable(handle_, chunk_rows, max_nq, cap_, mem_.device()); }
    std::optional<Tensor> split_scratch() const { return split_.tensor(); }
    std::tuple<Tensor, Tensor, Tensor> split_partials(int64_t Nq) const {
        return split_.partials(handle_, Nq, B_, cap_, d_model_, num_heads_);
    }

    // attend_tokens with the key sweep in chunks and a combine pass (qmha_attend_cached_tokens_split)
    Tensor attend_tokens_split(const Tensor& Q, const Tensor& lens, std::optional<Tensor> out_opt) {
        auto Qc = rows(Q, "Q", d_model_);
        per_seq(lens, "lens");
        split_.ready(Qc.size(1), "attend_tokens_split");
        Tensor out = out_for(out_opt, Qc);
        const OnStream on = current_stream(mem_.device());
        const int st = qmha_attend_cached_tokens_split(handle_, Qc.data_ptr<float>(), out.data_ptr<float>(), static_cast<int>(Qc.size(1)),
                                                       lens.data_ptr<int32_t>(), static_cast<int>(split_.chunk_rows),
                                                       split_.scratch.data_ptr(), static_cast<size_t>(split_.scratch.numel()),
                                                       QMHA_FLAG_CAUSAL, on.stream);
        TORCH_CHECK(st == QMHA_OK, "KVCache.attend_tokens_split", "(", kernel_, "): ", qmha_status_string(st), ": ", qmha_last_error());
        return out_opt ? out : out.view(Q.sizes());
    }

    // append_tokens with a row count per sequence (qmha_kv_cache_append_packed): K, V [total, num_kv_heads * d], cu int32 [B + 1]
    void append_packed(const Tensor& K, const Tensor& V, const Tensor& cu, const Tensor& pos, int64_t max_n) {
        auto Kc = cache_packed_rows(K, "K", kv_model_, mem_.device()), Vc = cache_packed_rows(V, "V", kv_model_, mem_.device());
        TORCH_CHECK(Kc.sizes() == Vc.sizes(), "K and V must have the same shape");
        cache_cu(cu, B_, mem_.device());
        per_seq(pos, "pos");
        const OnStream on = current_stream(mem_.device());
        const int st = qmha_kv_cache_append_packed(handle_, Kc.data_ptr<float>(), Vc.data_ptr<float>(), static_cast<int>(Kc.size(0)),
                                                   static_cast<int>(max_n), cu.data_ptr<int32_t>(), pos.data_ptr<int32_t>(), on.stream);
        TORCH_CHECK(st == QMHA_OK, "KVCache.append_packed", "(", kernel_, "): ", qmha_status_string(st), ": ", qmha_last_error());
    }

    // attend_tokens with a query count per sequence (qmha_attend_cached_packed): Q [total, d_model], cu int32 [B + 1]
    Tensor attend_packed(const Tensor& Q, const Tensor& cu, const Tensor& lens, int64_t max_nq, std::optional<Tensor> out_opt) {
        auto Qc = cache_packed_rows(Q, "Q", d_model_, mem_.device());
        cache_cu(cu, B_, mem_.device());
        per_seq(lens, "lens");
        Tensor out = packed_out(out_opt, Qc);
        const OnStream on = current_stream(mem_.device());
        const int st = qmha_attend_cached_packed(handle_, Qc.data_ptr<float>(), out.data_ptr<float>(), static_cast<int>(Qc.size(0)),
                                                 static_cast<int>(max_nq), cu.data_ptr<int32_t>(), lens.data_ptr<int32_t>(),
                                                 QMHA_FLAG_CAUSAL, on.stream);
        TORCH_CHECK(st == QMHA_OK, "KVCache.attend_packed", "(", kernel_, "): ", qmha_status_string(st), ": ", qmha_last_error());
        return out;
    }

private:
    void per_seq(const Tensor& t, const char* name) const { cache_per_seq(t, name, B_, mem_.device()); }
    Tensor rows(const Tensor& X, const char* name, int64_t width) const { return cache_rows(X, name, width, B_, mem_.device()); }
    int64_t B_, cap_, d_model_, kv_model_, num_heads_;
    std::string kernel_;
    Tensor mem_, tail_;
    SplitState split_;
    qmha_kv_cache_t* handle_ = nullptr;
};

// KVCache over num_kv_heads K/V heads (qmha_kv_cache_create_gqa): a class of its own, KVCache keeps its argument list
class GroupedKVCache : public KVCache {
public:
    GroupedKVCache(int64_t B, int64_t cap, int64_t d_model, int64_t num_heads, std::optional<int64_t> num_kv_heads,
                   const std::string& kernel, const std::string& device)
        : KVCache(B, cap, d_model, num_heads, kernel, device, num_kv_heads) {}
};

// A paged K/V cache (qmha_kv_cache_create_paged): the compiled form of quantizedmha_amd/torch_ext.py's PagedKVCache.  Owns
// the pool (a uint8 tensor of qmha_kv_cache_paged_bytes) and the host handle; the block table is the caller's tensor.
class PagedKVCache {
public:
    PagedKVCache(int64_t B, int64_t num_pages, int64_t page_rows, int64_t max_pages, int64_t d_model, int64_t num_heads,
                 std::optional<int64_t> num_kv_heads, const std::string& kernel, const std::string& device)
        : B_(B), max_pages_(max_pages), cap_(max_pages * page_rows), d_model_(d_model), kv_model_(d_model), num_heads_(num_heads),
          kernel_(kernel) {
        const int variant = qmha_variant_from_name(kernel.c_str());
        TORCH_CHECK(variant >= 0, "PagedKVCache: unknown kernel '", kernel, "'");
        c10::Device dev(device);
        TORCH_CHECK(dev.is_cuda(), "PagedKVCache needs a CUDA device");
        const int64_t h_kv = num_kv_heads ? *num_kv_heads : num_heads;
        if (num_heads > 0 && d_model % num_heads == 0) kv_model_ = h_kv * (d_model / num_heads);  // a bad head count: the library's checks
        const size_t bytes = qmha_kv_cache_paged_bytes(static_cast<int>(num_pages), static_cast<int>(page_rows), static_cast<int>(d_model),
                                                       static_cast<int>(num_heads), static_cast<int>(h_kv), variant);
        mem_ = torch::zeros({static_cast<int64_t>(bytes > 0 ? bytes : 1)}, torch::TensorOptions().dtype(torch::kUInt8).device(dev));
        const int st = qmha_kv_cache_create_paged(&handle_, mem_.data_ptr(), bytes, static_cast<int>(B), static_cast<int>(num_pages),
                                                  static_cast<int>(page_rows), static_cast<int>(max_pages), static_cast<int>(d_model),
                                                  static_cast<int>(num_heads), static_cast<int>(h_kv), variant);
        TORCH_CHECK(st == QMHA_OK, "PagedKVCache", "(", kernel, "): ", qmha_status_string(st), ": ", qmha_last_error());
    }
    ~PagedKVCache() { qmha_kv_cache_destroy(handle_); }
    PagedKVCache(const PagedKVCache&) = delete;
    PagedKVCache& operator=(const PagedKVCache&) = delete;

    int64_t cap() const { return cap_; }
    Tensor mem() const { return mem_; }
    std::optional<Tensor> tail() const { return tail_.defined() ? std::optional<Tensor>(tail_) : std::nullopt; }

    // allocate and attach the tail of raw rows append_paged needs (int8); once, outside a capture
    void enable_tokens() {
        if (tail_.defined()) return;
        const size_t bytes = qmha_kv_cache_tail_bytes(handle_);
        tail_ = torch::zeros({static_cast<int64_t>(bytes > 0 ? bytes : 1)}, torch::TensorOptions().dtype(torch::kUInt8).device(mem_.device()));
        const int st = qmha_kv_cache_attach_tail(handle_, tail_.data_ptr(), bytes);
        TORCH_CHECK(st == QMHA_OK, "PagedKVCache.enable_tokens", "(", kernel_, "): ", qmha_status_string(st), ": ", qmha_last_error());
    }

    // append_tokens through the block table (qmha_kv_cache_append_paged)
    void append_paged(const Tensor& K, const Tensor& V, const Tensor& pos, const Tensor& table) {
        auto Kc = cache_rows(K, "K", kv_model_, B_, mem_.device()), Vc = cache_rows(V, "V", kv_model_, B_, mem_.device());
        TORCH_CHECK(Kc.sizes() == Vc.sizes(), "K and V must have the same shape");
        cache_per_seq(pos, "pos", B_, mem_.device());
        check_table(table);
        const OnStream on = current_stream(mem_.device());
        const int st = qmha_kv_cache_append_paged(handle_, Kc.data_ptr<float>(), Vc.data_ptr<float>(), static_cast<int>(Kc.size(1)),
                                                  pos.data_ptr<int32_t>(), table.data_ptr<int32_t>(), on.stream);
        TORCH_CHECK(st == QMHA_OK, "PagedKVCache.append_paged", "(", kernel_, "): ", qmha_status_string(st), ": ", qmha_last_error());
    }

    // attend_tokens through the block table (qmha_attend_cached_paged)
    Tensor attend_paged(const Tensor& Q, const Tensor& lens, const Tensor& table, std::optional<Tensor> out_opt) {
        auto Qc = cache_rows(Q, "Q", d_model_, B_, mem_.device());
        cache_per_seq(lens, "lens", B_, mem_.device());
        check_table(table);
        Tensor out = out_for(out_opt, Qc);
        const OnStream on = current_stream(mem_.device());
        const int st = qmha_attend_cached_paged(handle_, Qc.data_ptr<float>(), out.data_ptr<float>(), static_cast<int>(Qc.size(1)),
                                                lens.data_ptr<int32_t>(), table.data_ptr<int32_t>(), QMHA_FLAG_CAUSAL, on.stream);
        TORCH_CHECK(st == QMHA_OK, "PagedKVCache.attend_paged", "(", kernel_, "): ", qmha_status_string(st), ": ", qmha_last_error());
        return out_opt ? out : out.view(Q.sizes());
    }

    // attend_tokens_window through the block table (qmha_attend_cached_paged_window)
    Tensor attend_paged_window(const Tensor& Q, const Tensor& lens, const Tensor& table, int64_t window, std::optional<Tensor> out_opt) {
        auto Qc = cache_rows(Q, "Q", d_model_, B_, mem_.device());
        cache_per_seq(lens, "lens", B_, mem_.device());
        check_table(table);
        TORCH_CHECK(window >= INT_MIN && window <= INT_MAX, "attend_paged_window: window = ", window, " does not fit an int");
        Tensor out = out_for(out_opt, Qc);
        const OnStream on = current_stream(mem_.device());
        const int st = qmha_attend_cached_paged_window(handle_, Qc.data_ptr<float>(), out.data_ptr<float>(), static_cast<int>(Qc.size(1)),
                                                       lens.data_ptr<int32_t>(), table.data_ptr<int32_t>(), static_cast<int>(window),
                                                       QMHA_FLAG_CAUSAL, on.stream);
        TORCH_CHECK(st == QMHA_OK, "PagedKVCache.attend_paged_window", "(", kernel_, "): ", qmha_status_string(st), ": ", qmha_last_error());
        return out_opt ? out : out.view(Q.sizes());
    }

    // the split-KV scratch, as KVCache's
    void enable_split(int64_t chunk_rows, int64_t max_nq) { split_.enable(handle_, chunk_rows, max_nq, cap_, mem_.device()); }
    std::optional<Tensor> split_scratch() const { return split_.tensor(); }
    std::tuple<Tensor, Tensor, Tensor> split_partials(int64_t Nq) const {
        return split_.partials(handle_, Nq, B_, cap_, d_model_, num_heads_);
    }

    // attend_tokens_split through the block table (qmha_attend_cached_paged_split)
    Tensor attend_paged_split(const Tensor& Q, const Tensor& lens, const Tensor& table, std::optional<Tensor> out_opt) {
        auto Qc = cache_rows(Q, "Q", d_model_, B_, mem_.device());
        cache_per_seq(lens, "lens", B_, mem_.device());
        check_table(table);
        split_.ready(Qc.size(1), "attend_paged_split");
        Tensor out = out_for(out_opt, Qc);
        const OnStream on = current_stream(mem_.device());
        const int st = qmha_attend_cached_paged_split(handle_, Qc.data_ptr<float>(), out.data_ptr<float>(), static_cast<int>(Qc.size(1)),
                                                      lens.data_ptr<int32_t>(), table.data_ptr<int32_t>(), static_cast<int>(split_.chunk_rows),
                                                      split_.scratch.data_ptr(), static_cast<size_t>(split_.scratch.numel()),
                                                      QMHA_FLAG_CAUSAL, on.stream);
        TORCH_CHECK(st == QMHA_OK, "PagedKVCache.attend_paged_split", "(", kernel_, "): ", qmha_status_string(st), ": ", qmha_last_error());
        return out_opt ? out : out.view(Q.sizes());
    }

    // append_packed through the block table (qmha_kv_cache_append_paged_packed)
    void append_paged_packed(const Tensor& K, const Tensor& V, const Tensor& cu, const Tensor& pos, const Tensor& table, int64_t max_n) {
        auto Kc = cache_packed_rows(K, "K", kv_model_, mem_.device()), Vc = cache_packed_rows(V, "V", kv_model_, mem_.device());
        TORCH_CHECK(Kc.sizes() == Vc.sizes(), "K and V must have the same shape");
        cache_cu(cu, B_, mem_.device());
        cache_per_seq(pos, "pos", B_, mem_.device());
        check_table(table);
        const OnStream on = current_stream(mem_.device());
        const int st = qmha_kv_cache_append_paged_packed(handle_, Kc.data_ptr<float>(), Vc.data_ptr<float>(), static_cast<int>(Kc.size(0)),
                                                         static_cast<int>(max_n), cu.data_ptr<int32_t>(), pos.data_ptr<int32_t>(),
                                                         table.data_ptr<int32_t>(), on.stream);
        TORCH_CHECK(st == QMHA_OK, "PagedKVCache.append_paged_packed", "(", kernel_, "): ", qmha_status_string(st), ": ", qmha_last_error());
    }

    // attend_packed through the block table (qmha_attend_cached_paged_packed)
    Tensor attend_paged_packed(const Tensor& Q, const Tensor& cu, const Tensor& lens, const Tensor& table, int64_t max_nq,
                               std::optional<Tensor> out_opt) {
        auto Qc = cache_packed_rows(Q, "Q", d_model_, mem_.device());
        cache_cu(cu, B_, mem_.device());
        cache_per_seq(lens, "lens", B_, mem_.device());
        check_table(table);
        Tensor out = packed_out(out_opt, Qc);
        const OnStream on = current_stream(mem_.device());
        const int st = qmha_attend_cached_paged_packed(handle_, Qc.data_ptr<float>(), out.data_ptr<float>(), static_cast<int>(Qc.size(0)),
                                                       static_cast<int>(max_nq), cu.data_ptr<int32_t>(), lens.data_ptr<int32_t>(),
                                                       table.data_ptr<int32_t>(), QMHA_FLAG_CAUSAL, on.stream);
        TORCH_CHECK(st == QMHA_OK, "PagedKVCache.attend_paged_packed", "(", kernel_, "): ", qmha_status_string(st), ": ", qmha_last_error());
        return out;
    }

private:
    // the block table: int32 [B, max_pages] on the cache's device, contiguous: the kernel reads it, the host does not
    void check_table(const Tensor& t) const {
        TORCH_CHECK(t.is_cuda(), "table must be a CUDA tensor");
        TORCH_CHECK(t.dtype() == torch::kInt32, "table must be int32");
        TORCH_CHECK(t.device() == mem_.device(), "table must be on the cache's device");
        TORCH_CHECK(t.dim() == 2 && t.size(0) == B_ && t.size(1) == max_pages_ && t.is_contiguous(),
                    "table must be a contiguous tensor of shape [B = ", B_, ", max_pages = ", max_pages_, "]");
    }
    int64_t B_, max_pages_, cap_, d_model_, kv_model_, num_heads_;
    std::string kernel_;
    Tensor mem_, tail_;
    SplitState split_;
    qmha_kv_cache_t* handle_ = nullptr;
};

PYBIND11_MODULE(torch_ext, m) {
    pybind11::class_<PagedKVCache>(m, "PagedKVCache",
                                   "Paged K/V cache (HIP, MI355X): a pool of num_pages pages of page_rows rows and a caller-owned int32\n"
                                   "[B, max_pages] block table on the device; append_paged / attend_paged are append_tokens /\n"
                                   "attend_tokens with the row looked up through the table.")
        .def(pybind11::init<int64_t, int64_t, int64_t, int64_t, int64_t, int64_t, std::optional<int64_t>, const std::string&,
                            const std::string&>(),
             pybind11::arg("B"), pybind11::arg("num_pages"), pybind11::arg("page_rows"), pybind11::arg("max_pages"), pybind11::arg("d_model"),
             pybind11::arg("num_heads"), pybind11::arg("num_kv_heads") = pybind11::none(), pybind11::arg("kernel") = "fa_tc_int8_b",
             pybind11::arg("device") = "cuda")
        .def("enable_tokens", &PagedKVCache::enable_tokens,
             "allocate and attach the tail of raw rows append_paged needs (int8); once, outside a graph capture.")
        .def("append_paged", &PagedKVCache::append_paged, pybind11::arg("K"), pybind11::arg("V"), pybind11::arg("pos"),
             pybind11::arg("table"),
             "append_tokens through the table: sequence b's n >= 1 rows go to logical rows [pos[b], pos[b] + n); an invalid pos[b]\n"
             "or a touched table entry outside [0, num_pages) writes nothing for that sequence.")
        .def("attend_paged", &PagedKVCache::attend_paged, pybind11::arg("Q"), pybind11::arg("lens"), pybind11::arg("table"),
             pybind11::arg("out") = pybind11::none(),
             "attend_tokens through the table; an invalid lens[b] or a used table entry outside [0, num_pages) gives zeros.")
        .def("attend_paged_window", &PagedKVCache::attend_paged_window, pybind11::arg("Q"), pybind11::arg("lens"), pybind11::arg("table"),
             pybind11::arg("window"), pybind11::arg("out") = pybind11::none(),
             "attend_tokens_window through the table, bit for bit; table columns behind the window's pages are not read.")
        .def("enable_split", &PagedKVCache::enable_split, pybind11::arg("chunk_rows"), pybind11::arg("max_nq") = 32,
             "allocate the scratch of attend_paged_split for chunks of chunk_rows key rows (a multiple of 64) and up to max_nq\n"
             "query rows; once, outside a graph capture.")
        .def("attend_paged_split", &PagedKVCache::attend_paged_split, pybind11::arg("Q"), pybind11::arg("lens"), pybind11::arg("table"),
             pybind11::arg("out") = pybind11::none(),
             "attend_paged with the key sweep in chunks and a combine pass: attend_tokens_split through the table, bit for bit.")
        .def("split_partials", &PagedKVCache::split_partials, pybind11::arg("Nq"),
             "(Oc, m, l) views of the scratch: what the last split attend of Nq rows left per chunk.")
        .def("append_paged_packed", &PagedKVCache::append_paged_packed, pybind11::arg("K"), pybind11::arg("V"), pybind11::arg("cu"),
             pybind11::arg("pos"), pybind11::arg("table"), pybind11::arg("max_n"),
             "append_paged with a row count per sequence: K, V [total, num_kv_heads * d], rows [cu[b], cu[b + 1]) are sequence b's;\n"
             "cu: int32 [B + 1] on the device, read by the kernel; max_n: an upper bound of the counts.")
        .def("attend_paged_packed", &PagedKVCache::attend_paged_packed, pybind11::arg("Q"), pybind11::arg("cu"), pybind11::arg("lens"),
             pybind11::arg("table"), pybind11::arg("max_nq"), pybind11::arg("out") = pybind11::none(),
             "attend_paged with a query count per sequence: Q [total, d_model], rows [cu[b], cu[b + 1]) are sequence b's;\n"
             "max_nq: an upper bound of the counts.")
        .def_property_readonly("split_scratch", &PagedKVCache::split_scratch)
        .def_property_readonly("tail", &PagedKVCache::tail)
        .def_property_readonly("cap", &PagedKVCache::cap)
        .def_property_readonly("mem", &PagedKVCache::mem);
    pybind11::class_<KVCache>(m, "KVCache",
                              "Persistent quantised K/V cache (HIP, MI355X): append(K, V) pre-passes new rows into place,\n"
                              "attend(Q, causal=True) attends the last Nq positions over the cached rows.")
        .def(pybind11::init<int64_t, int64_t, int64_t, int64_t, const std::string&, const std::string&>(), pybind11::arg("B"),
             pybind11::arg("cap"), pybind11::arg("d_model"), pybind11::arg("num_heads"), pybind11::arg("kernel") = "fa_tc_int8_b",
             pybind11::arg("device") = "cuda")
        .def("append", &KVCache::append, pybind11::arg("K"), pybind11::arg("V"))
        .def("attend", &KVCache::attend, pybind11::arg("Q"), pybind11::arg("causal") = true)
        .def("truncate", &KVCache::truncate, pybind11::arg("n"))
        .def("append_at", &KVCache::append_at, pybind11::arg("K"), pybind11::arg("V"), pybind11::arg("pos"),
             "append with a row per sequence: sequence b's rows go to cache rows [pos[b], pos[b] + n); pos: int32 [B] on the\n"
             "device, read by the kernel; an invalid pos[b] writes nothing for that sequence.")
        .def("attend_varlen", &KVCache::attend_varlen, pybind11::arg("Q"), pybind11::arg("lens"), pybind11::arg("causal") = true,
             pybind11::arg("out") = pybind11::none(),
             "attend with a length per sequence: sequence b attends its first lens[b] cache rows; lens: int32 [B] on the\n"
             "device, read by the kernel; an invalid lens[b] gives zeros for that sequence.")
        .def("enable_tokens", &KVCache::enable_tokens,
             "allocate and attach the tail of raw rows append_tokens needs (int8); once, outside a graph capture.")
        .def("append_tokens", &KVCache::append_tokens, pybind11::arg("K"), pybind11::arg("V"), pybind11::arg("pos"),
             "append_at for any number of rows n >= 1 at any row pos[b]; the touched 32-row groups hold what append_at writes\n"
             "for their rows so far, zero-padded; an invalid pos[b] writes nothing for that sequence.")
        .def("attend_tokens", &KVCache::attend_tokens, pybind11::arg("Q"), pybind11::arg("lens"), pybind11::arg("out") = pybind11::none(),
             "causal attend_varlen for any Nq >= 1 and any lens[b] in [Nq, cap]; an invalid lens[b] gives zeros.")
        .def("attend_tokens_window", &KVCache::attend_tokens_window, pybind11::arg("Q"), pybind11::arg("lens"), pybind11::arg("window"),
             pybind11::arg("out") = pybind11::none(),
             "attend_tokens over the last `window` keys of a row (a multiple of 32, >= 32); window >= cap gives attend_tokens' bits.")
        .def("enable_split", &KVCache::enable_split, pybind11::arg("chunk_rows"), pybind11::arg("max_nq") = 32,
             "allocate the scratch of attend_tokens_split for chunks of chunk_rows key rows (a multiple of 64) and up to max_nq\n"
             "query rows; once, outside a graph capture.")
        .def("attend_tokens_split", &KVCache::attend_tokens_split, pybind11::arg("Q"), pybind11::arg("lens"),
             pybind11::arg("out") = pybind11::none(),
             "attend_tokens with the key sweep in chunks and a combine pass, for a decode step on long sequences.")
        .def("split_partials", &KVCache::split_partials, pybind11::arg("Nq"),
             "(Oc, m, l) views of the scratch: what the last split attend of Nq rows left per chunk.")
        .def("append_packed", &KVCache::append_packed, pybind11::arg("K"), pybind11::arg("V"), pybind11::arg("cu"), pybind11::arg("pos"),
             pybind11::arg("max_n"),
             "append_tokens with a row count per sequence: K, V [total, num_kv_heads * d], rows [cu[b], cu[b + 1]) are sequence b's;\n"
             "cu: int32 [B + 1] on the device, read by the kernel; max_n: an upper bound of the counts.")
        .def("attend_packed", &KVCache::attend_packed, pybind11::arg("Q"), pybind11::arg("cu"), pybind11::arg("lens"),
             pybind11::arg("max_nq"), pybind11::arg("out") = pybind11::none(),
             "attend_tokens with a query count per sequence: Q [total, d_model], rows [cu[b], cu[b + 1]) are sequence b's;\n"
             "max_nq: an upper bound of the counts.")
        .def_property_readonly("split_scratch", &KVCache::split_scratch)
        .def_property_readonly("tail", &KVCache::tail)
        .def_property_readonly("len", &KVCache::len)
        .def_property_readonly("cap", &KVCache::cap)
        .def_property_readonly("mem", &KVCache::mem);
    pybind11::class_<GroupedKVCache, KVCache>(m, "GroupedKVCache",
                                              "KVCache for grouped-query attention: num_kv_heads K/V heads shared by the num_heads\n"
                                              "query heads; append(K, V) takes [B, n, num_kv_heads * d].")
        .def(pybind11::init<int64_t, int64_t, int64_t, int64_t, std::optional<int64_t>, const std::string&, const std::string&>(),
             pybind11::arg("B"), pybind11::arg("cap"), pybind11::arg("d_model"), pybind11::arg("num_heads"),
             pybind11::arg("num_kv_heads") = pybind11::none(), pybind11::arg("kernel") = "fa_tc_int8_b",
             pybind11::arg("device") = "cuda");
    m.def("flash_solve_gqa", &flash_solve_gqa,
          "FlashAttention solve with grouped K/V heads and separate query and key lengths (HIP, MI355X)\n\n"
          "Args:\n"
          "  Q: Query tensor [Nq, d_model] (or [B, Nq, d_model])\n"
          "  K: Key tensor [Nk, num_kv_heads * d] (or [B, Nk, num_kv_heads * d]), d = d_model / num_heads\n"
          "  V: Value tensor, shaped like K\n"
          "  d_model: Model dimension\n"
          "  num_heads: Number of query heads\n"
          "  num_kv_heads: Number of K/V heads, a divisor of num_heads (default: None = num_heads)\n"
          "  kernel: Kernel variant (default: 'fa_tc_int8_b')\n"
          "  causal: bottom-right aligned, query row r attends keys j <= r + (Nk - Nq) (default: False)",
          pybind11::arg("Q"), pybind11::arg("K"), pybind11::arg("V"), pybind11::arg("d_model"),
          pybind11::arg("num_heads"), pybind11::arg("num_kv_heads") = pybind11::none(),
          pybind11::arg("kernel") = "fa_tc_int8_b", pybind11::arg("causal") = false);
    m.def("flash_solve_rect", &flash_solve_rect,
          "FlashAttention solve with separate query and key lengths (HIP, MI355X)\n\n"
          "Args:\n"
          "  Q: Query tensor [Nq, d_model] (or [B, Nq, d_model])\n"
          "  K: Key tensor [Nk, d_model] (or [B, Nk, d_model])\n"
          "  V: Value tensor, shaped like K\n"
          "  d_model: Model dimension\n"
          "  num_heads: Number of attention heads\n"
          "  kernel: Kernel variant (default: 'fa_tc_int8_b')\n"
          "  causal: bottom-right aligned, query row r attends keys j <= r + (Nk - Nq) (default: False)",
          pybind11::arg("Q"), pybind11::arg("K"), pybind11::arg("V"), pybind11::arg("d_model"),
          pybind11::arg("num_heads"), pybind11::arg("kernel") = "fa_tc_int8_b", pybind11::arg("causal") = false);
    m.def("flash_solve", &flash_solve,
          "FlashAttention solve (HIP, MI355X)\n\n"
          "Args:\n"
          "  Q: Query tensor [N, d_model] (or [B, N, d_model])\n"
          "  K: Key tensor [N, d_model]\n"
          "  V: Value tensor [N, d_model]\n"
          "  d_model: Model dimension\n"
          "  num_heads: Number of attention heads\n"
          "  kernel: Kernel variant (default: 'fa_tc_int8_b')\n"
          "  causal: query row r attends keys j <= r (default: False)",
          pybind11::arg("Q"), pybind11::arg("K"), pybind11::arg("V"), pybind11::arg("d_model"),
          pybind11::arg("num_heads"), pybind11::arg("kernel") = "fa_tc_int8_b", pybind11::arg("causal") = false);
}
