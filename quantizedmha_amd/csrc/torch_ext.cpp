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
//   * a rejected shape raises (TORCH_CHECK on the C-ABI status) instead of a device assert.
#include <torch/extension.h>
// ROCm PyTorch reports HIP devices as device type "cuda": the guard / current-stream
// accessors for such tensors are the "MasqueradingAsCUDA" ones
#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>

#include <string>

#include "launchers.h"

using torch::Tensor;

static Tensor flash_solve(const Tensor& Q, const Tensor& K, const Tensor& V, int64_t d_model, int64_t num_heads,
                          const std::string& kernel = "fa_tc_int8_b", bool causal = false) {
    TORCH_CHECK(Q.is_cuda() && K.is_cuda() && V.is_cuda(), "Inputs must be CUDA tensors");
    TORCH_CHECK(Q.dtype() == torch::kFloat32, "Q must be float32");
    TORCH_CHECK(K.dtype() == torch::kFloat32, "K must be float32");
    TORCH_CHECK(V.dtype() == torch::kFloat32, "V must be float32");
    auto Qc = Q.contiguous();
    auto Kc = K.contiguous();
    auto Vc = V.contiguous();
    const int64_t q_elems = Qc.numel();
    TORCH_CHECK(d_model > 0 && q_elems % d_model == 0, "Q.numel() must be divisible by d_model");
    TORCH_CHECK(Kc.sizes() == Qc.sizes() && Vc.sizes() == Qc.sizes(), "Q, K and V must have the same shape");
    // [B, N, d_model] is B sequences; any other layout is one sequence of numel / d_model rows,
    // as in the reference (torch_ext.cpp:23-25), e.g. [N, h, d]
    const bool batched = Qc.dim() == 3 && Qc.size(2) == d_model;
    const int64_t B = batched ? Qc.size(0) : 1;
    const int64_t N = batched ? Qc.size(1) : q_elems / d_model;
    int variant = qmha_variant_from_name(kernel.c_str());
    if (variant < 0) {
        TORCH_WARN("Kernel selection supports fa, fa_tc_v1a, fa_tc_int8_b, unfused, fa_mfma, fa_tc_int8_pt; '", kernel,
                   "' routing to default 'fa_tc_int8_b'");
        variant = QMHA_FA_TC_INT8_B;
    }
    auto out = torch::empty_like(Qc);
    const c10::hip::HIPGuardMasqueradingAsCUDA guard(Qc.device());
    const hipStream_t stream = c10::hip::getCurrentHIPStreamMasqueradingAsCUDA(Qc.device().index()).stream();
    // causal = false enqueues exactly what qmha_solve_ex does (flags == 0)
    const int st = qmha_solve_opts(Qc.data_ptr<float>(), Kc.data_ptr<float>(), Vc.data_ptr<float>(),
                                   out.data_ptr<float>(), static_cast<int>(B), static_cast<int>(N),
                                   static_cast<int>(d_model), static_cast<int>(num_heads), variant,
                                   causal ? QMHA_FLAG_CAUSAL : 0u, nullptr, 0, stream);
    TORCH_CHECK(st == QMHA_OK, "flash_solve(", kernel, "): ", qmha_status_string(st), ": ", qmha_last_error());
    return out;
}

// flash_solve with a query length of its own (qmha_solve_rect): K and V share one shape, Q has its own row
// count and the same batch count; the result is shaped like Q.  causal: bottom-right aligned.
static Tensor flash_solve_rect(const Tensor& Q, const Tensor& K, const Tensor& V, int64_t d_model, int64_t num_heads,
                               const std::string& kernel = "fa_tc_int8_b", bool causal = false) {
    TORCH_CHECK(Q.is_cuda() && K.is_cuda() && V.is_cuda(), "Inputs must be CUDA tensors");
    TORCH_CHECK(Q.dtype() == torch::kFloat32, "Q must be float32");
    TORCH_CHECK(K.dtype() == torch::kFloat32, "K must be float32");
    TORCH_CHECK(V.dtype() == torch::kFloat32, "V must be float32");
    auto Qc = Q.contiguous();
    auto Kc = K.contiguous();
    auto Vc = V.contiguous();
    TORCH_CHECK(d_model > 0 && Qc.numel() % d_model == 0, "Q.numel() must be divisible by d_model");
    TORCH_CHECK(Kc.sizes() == Vc.sizes(), "K and V must have the same shape");
    TORCH_CHECK(Kc.numel() % d_model == 0, "K.numel() must be divisible by d_model");
    const auto rows = [d_model](const Tensor& t, int64_t* B) {  // flash_solve's shape rule
        const bool batched = t.dim() == 3 && t.size(2) == d_model;
        *B = batched ? t.size(0) : 1;
        return batched ? t.size(1) : t.numel() / d_model;
    };
    int64_t B = 1, Bk = 1;
    const int64_t Nq = rows(Qc, &B), Nk = rows(Kc, &Bk);
    TORCH_CHECK(B == Bk, "Q and K must have the same batch count");
    int variant = qmha_variant_from_name(kernel.c_str());
    if (variant < 0) {
        TORCH_WARN("Kernel selection supports fa, fa_tc_v1a, fa_tc_int8_b, unfused, fa_mfma, fa_tc_int8_pt; '", kernel,
                   "' routing to default 'fa_tc_int8_b'");
        variant = QMHA_FA_TC_INT8_B;
    }
    auto out = torch::empty_like(Qc);
    const c10::hip::HIPGuardMasqueradingAsCUDA guard(Qc.device());
    const hipStream_t stream = c10::hip::getCurrentHIPStreamMasqueradingAsCUDA(Qc.device().index()).stream();
    const int st = qmha_solve_rect(Qc.data_ptr<float>(), Kc.data_ptr<float>(), Vc.data_ptr<float>(),
                                   out.data_ptr<float>(), static_cast<int>(B), static_cast<int>(Nq), static_cast<int>(Nk),
                                   static_cast<int>(d_model), static_cast<int>(num_heads), variant,
                                   causal ? QMHA_FLAG_CAUSAL : 0u, nullptr, 0, stream);
    TORCH_CHECK(st == QMHA_OK, "flash_solve_rect(", kernel, "): ", qmha_status_string(st), ": ", qmha_last_error());
    return out;
}

// A persistent quantised K/V cache (qmha_kv_cache_*): the compiled form of quantizedmha_amd/torch_ext.py's KVCache.
// Owns a uint8 tensor of qmha_kv_cache_bytes and the host handle; append / attend run on PyTorch's current stream.
class KVCache {
public:
    KVCache(int64_t B, int64_t cap, int64_t d_model, int64_t num_heads, const std::string& kernel, const std::string& device)
        : B_(B), cap_(cap), d_model_(d_model), kernel_(kernel) {
        const int variant = qmha_variant_from_name(kernel.c_str());
        TORCH_CHECK(variant >= 0, "KVCache: unknown kernel '", kernel, "'");
        c10::Device dev(device);
        TORCH_CHECK(dev.is_cuda(), "KVCache needs a CUDA device");
        const size_t bytes = qmha_kv_cache_bytes(static_cast<int>(B), static_cast<int>(cap), static_cast<int>(d_model),
                                                 static_cast<int>(num_heads), variant);
        mem_ = torch::zeros({static_cast<int64_t>(bytes > 0 ? bytes : 1)}, torch::TensorOptions().dtype(torch::kUInt8).device(dev));
        const int st = qmha_kv_cache_create(&handle_, mem_.data_ptr(), bytes, static_cast<int>(B), static_cast<int>(cap),
                                            static_cast<int>(d_model), static_cast<int>(num_heads), variant);
        TORCH_CHECK(st == QMHA_OK, "KVCache(", kernel, "): ", qmha_status_string(st), ": ", qmha_last_error());
    }
    ~KVCache() { qmha_kv_cache_destroy(handle_); }
    KVCache(const KVCache&) = delete;
    KVCache& operator=(const KVCache&) = delete;

    int64_t len() const { return qmha_kv_cache_len(handle_); }
    int64_t cap() const { return cap_; }
    Tensor mem() const { return mem_; }

    void append(const Tensor& K, const Tensor& V) {
        auto Kc = rows(K, "K"), Vc = rows(V, "V");
        TORCH_CHECK(Kc.sizes() == Vc.sizes(), "K and V must have the same shape");
        const c10::hip::HIPGuardMasqueradingAsCUDA guard(mem_.device());
        const hipStream_t stream = c10::hip::getCurrentHIPStreamMasqueradingAsCUDA(mem_.device().index()).stream();
        const int st = qmha_kv_cache_append(handle_, Kc.data_ptr<float>(), Vc.data_ptr<float>(), static_cast<int>(Kc.size(1)), stream);
        TORCH_CHECK(st == QMHA_OK, "KVCache.append(", kernel_, "): ", qmha_status_string(st), ": ", qmha_last_error());
    }

    Tensor attend(const Tensor& Q, bool causal) {
        auto Qc = rows(Q, "Q");
        auto out = torch::empty_like(Qc);
        const c10::hip::HIPGuardMasqueradingAsCUDA guard(mem_.device());
        const hipStream_t stream = c10::hip::getCurrentHIPStreamMasqueradingAsCUDA(mem_.device().index()).stream();
        const int st = qmha_attend_cached(handle_, Qc.data_ptr<float>(), out.data_ptr<float>(), static_cast<int>(Qc.size(1)),
                                          causal ? QMHA_FLAG_CAUSAL : 0u, stream);
        TORCH_CHECK(st == QMHA_OK, "KVCache.attend(", kernel_, "): ", qmha_status_string(st), ": ", qmha_last_error());
        return out.view(Q.sizes());
    }

    void truncate(int64_t n) {
        const int st = qmha_kv_cache_truncate(handle_, static_cast<int>(n));
        TORCH_CHECK(st == QMHA_OK, "KVCache.truncate: ", qmha_status_string(st), ": ", qmha_last_error());
    }

private:
    // [B, n, d_model] fp32 on the cache's device, contiguous; [n, d_model] for B = 1
    Tensor rows(const Tensor& X, const char* name) const {
        TORCH_CHECK(X.is_cuda(), "Inputs must be CUDA tensors");
        TORCH_CHECK(X.dtype() == torch::kFloat32, name, " must be float32");
        TORCH_CHECK(X.device() == mem_.device(), name, " must be on the cache's device");
        auto Xc = X.contiguous();
        if (Xc.dim() == 2 && B_ == 1) Xc = Xc.unsqueeze(0);
        TORCH_CHECK(Xc.dim() == 3 && Xc.size(0) == B_ && Xc.size(2) == d_model_, name, " must be [B = ", B_, ", n, d_model = ",
                    d_model_, "]", B_ == 1 ? " or [n, d_model]" : "");
        return Xc;
    }
    int64_t B_, cap_, d_model_;
    std::string kernel_;
    Tensor mem_;
    qmha_kv_cache_t* handle_ = nullptr;
};

PYBIND11_MODULE(torch_ext, m) {
    pybind11::class_<KVCache>(m, "KVCache",
                              "Persistent quantised K/V cache (HIP, MI355X): append(K, V) pre-passes new rows into place,\n"
                              "attend(Q, causal=True) attends the last Nq positions over the cached rows.")
        .def(pybind11::init<int64_t, int64_t, int64_t, int64_t, const std::string&, const std::string&>(), pybind11::arg("B"),
             pybind11::arg("cap"), pybind11::arg("d_model"), pybind11::arg("num_heads"), pybind11::arg("kernel") = "fa_tc_int8_b",
             pybind11::arg("device") = "cuda")
        .def("append", &KVCache::append, pybind11::arg("K"), pybind11::arg("V"))
        .def("attend", &KVCache::attend, pybind11::arg("Q"), pybind11::arg("causal") = true)
        .def("truncate", &KVCache::truncate, pybind11::arg("n"))
        .def_property_readonly("len", &KVCache::len)
        .def_property_readonly("cap", &KVCache::cap)
        .def_property_readonly("mem", &KVCache::mem);
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
