"""PyTorch binding: mirror of the reference's extensions/torch/torch_ext.cpp (torch_ext.flash_solve).

Same name, arguments, return value and error behaviour as the reference:
  flash_solve(Q, K, V, d_model, num_heads, kernel='fa_tc_int8_b') -> Tensor shaped like Q
  (additive trailing arguments: out=None, causal=False)
  * non-GPU inputs        -> RuntimeError("Inputs must be CUDA tensors")       (:14)
  * non-fp32 inputs       -> RuntimeError("Q must be float32") etc.            (:15-17)
  * numel % d_model != 0  -> RuntimeError("Q.numel() must be divisible by d_model")  (:24)
  * unknown kernel name   -> warning, routed to the default fa_tc_int8_b       (:32-34)
Differences (additive): `kernel` really selects the variant (the reference only warned and
used its build-time kernel); a 3-D input [B, N, d_model] is treated as B sequences (the
reference has no batch; any other shape is one sequence of numel/d_model rows, as there); K and V
must have Q's shape; work is enqueued on torch's current stream instead of private
streams + a blocking sync (torch orders it with surrounding ops on that stream).
ROCm tensors report device type 'cuda', exactly as the reference's is_cuda() check expects.
flash_solve_rect (additive, no reference counterpart) is flash_solve with a query length of its own: K and V
share one shape, Q has its own row count (cross-attention, chunked prefill; qmha_solve_rect).
KVCache (additive) keeps the pre-passed K and V of earlier chunks: append new rows, attend with the last Nq.
Both take num_kv_heads (additive, default None = num_heads): grouped-query attention, K and V of num_kv_heads heads.
"""
from __future__ import annotations

import contextlib
import ctypes
import warnings
from typing import Optional

import torch

from . import _lib


def _shape(Q: torch.Tensor, d_model: int):
    """(B, N): [B, N, d_model] is B sequences; any other layout is one sequence of
    numel / d_model rows, as in the reference (torch_ext.cpp:23-25), e.g. [N, h, d]."""
    n = Q.numel()
    if d_model <= 0 or n % d_model != 0:
        raise RuntimeError("Q.numel() must be divisible by d_model")
    if Q.dim() == 3 and Q.shape[2] == d_model:
        return Q.shape[0], Q.shape[1]
    return 1, n // d_model


def _fp32_inputs(Q: torch.Tensor, K: torch.Tensor, V: torch.Tensor):
    """Q, K, V made contiguous; all on the GPU and float32, or the reference's errors (torch_ext.cpp:14-17)."""
    if not (Q.is_cuda and K.is_cuda and V.is_cuda):
        raise RuntimeError("Inputs must be CUDA tensors")
    for name, t in (("Q", Q), ("K", K), ("V", V)):
        if t.dtype != torch.float32:
            raise RuntimeError(f"{name} must be float32")
    return Q.contiguous(), K.contiguous(), V.contiguous()


def _known_kernel(kernel: str) -> str:
    """An unknown kernel name warns and routes to the default (torch_ext.cpp:32-34)."""
    if kernel in _lib.VARIANTS:
        return kernel
    warnings.warn(f"Kernel selection supports {sorted(_lib.VARIANTS)}; '{kernel}' routing to default "
                  f"'{_lib.DEFAULT_KERNEL}'")
    return _lib.DEFAULT_KERNEL


def _out_for(out: Optional[torch.Tensor], Qc: torch.Tensor, same: str) -> torch.Tensor:
    """The caller's `out`, checked against Qc by shape or by size (numel), or a new tensor like Qc."""
    if out is None:
        return torch.empty_like(Qc)
    fits = out.shape == Qc.shape if same == "shape" else out.numel() == Qc.numel()
    if not fits or out.dtype != torch.float32 or out.device != Qc.device or not out.is_contiguous():
        raise RuntimeError(f"out must be a contiguous float32 tensor of Q's {same} on Q's device")
    return out


@contextlib.contextmanager
def _current_stream(device):
    """`device` made current; yields the handle of torch's current stream there."""
    with torch.cuda.device(device):
        yield torch.cuda.current_stream(device).cuda_stream


def flash_solve(Q: torch.Tensor, K: torch.Tensor, V: torch.Tensor, d_model: int, num_heads: int,
                kernel: str = _lib.DEFAULT_KERNEL, out: Optional[torch.Tensor] = None,
                causal: bool = False) -> torch.Tensor:
    """FlashAttention solve (HIP).  Q, K, V: [N, d_model] (or [B, N, d_model]) fp32 on the GPU.
    out (additive): a contiguous fp32 tensor of Q's shape on Q's device to write the result into
    (the batch-shard path writes each rank's rows straight into the gathered result).
    causal (additive): query row r attends keys j <= r of its own sequence (fa_tc_int8_b at
    d = 32 / 64 / 128, fa_tc_v1a at d = 64 / 128; anything else raises)."""
    Qc, Kc, Vc = _fp32_inputs(Q, K, V)
    d_model, num_heads = int(d_model), int(num_heads)
    B, N = _shape(Qc, d_model)
    if Kc.shape != Qc.shape or Vc.shape != Qc.shape:
        raise RuntimeError("Q, K and V must have the same shape")
    kernel = _known_kernel(kernel)
    out = _out_for(out, Qc, "shape")
    lib = _lib.load()
    with _current_stream(Qc.device) as stream:
        if causal:
            st = lib.qmha_solve_opts(Qc.data_ptr(), Kc.data_ptr(), Vc.data_ptr(), out.data_ptr(), B, N, d_model,
                                     num_heads, _lib.variant_id(kernel), _lib.QMHA_FLAG_CAUSAL, None, 0, stream)
        else:
            st = lib.qmha_solve_ex(Qc.data_ptr(), Kc.data_ptr(), Vc.data_ptr(), out.data_ptr(), B, N, d_model,
                                   num_heads, _lib.variant_id(kernel), stream)
    _lib.check(st, f"flash_solve({kernel})")
    return out


def flash_solve_rect(Q: torch.Tensor, K: torch.Tensor, V: torch.Tensor, d_model: int, num_heads: int,
                     kernel: str = _lib.DEFAULT_KERNEL, out: Optional[torch.Tensor] = None,
                     causal: bool = False) -> torch.Tensor:
    """flash_solve with a query length of its own (qmha_solve_rect): Q is [Nq, d_model] or [B, Nq, d_model],
    K and V share one shape [Nk, d_model] or [B, Nk, d_model] with Q's batch count; returns a tensor shaped
    like Q.  causal: bottom-right aligned, query row r attends keys j <= r + (Nk - Nq) (the Nq queries are the
    last Nq positions of a sequence of Nk; Nk >= Nq).  Nq != Nk: fa_tc_int8_b at d = 32 / 64 / 128 and
    fa_tc_v1a at d = 64 / 128; anything else raises.  Arguments and error behaviour as flash_solve."""
    return _solve_rect(Q, K, V, d_model, num_heads, None, kernel, out, causal, "flash_solve_rect")


def flash_solve_gqa(Q: torch.Tensor, K: torch.Tensor, V: torch.Tensor, d_model: int, num_heads: int,
                    num_kv_heads: Optional[int] = None, kernel: str = _lib.DEFAULT_KERNEL,
                    out: Optional[torch.Tensor] = None, causal: bool = False) -> torch.Tensor:
    """flash_solve_rect for grouped-query attention (qmha_solve_gqa): K and V are [Nk, num_kv_heads * d] or
    [B, Nk, num_kv_heads * d] (d = d_model / num_heads) and query head k reads K/V head
    k // (num_heads // num_kv_heads).  With fewer K/V heads than heads: fa_tc_int8_b at d = 32 / 64 / 128 and
    fa_tc_v1a at d = 64 / 128, for every Nq and Nk; anything else raises.  num_kv_heads = None is flash_solve_rect.
    (A function of its own: flash_solve_rect keeps the argument list its callers and tests know.)"""
    return _solve_rect(Q, K, V, d_model, num_heads, num_kv_heads, kernel, out, causal, "flash_solve_gqa")


def _solve_rect(Q, K, V, d_model, num_heads, num_kv_heads, kernel, out, causal, what):
    Qc, Kc, Vc = _fp32_inputs(Q, K, V)
    d_model, num_heads = int(d_model), int(num_heads)
    B, Nq = _shape(Qc, d_model)
    if Kc.shape != Vc.shape:
        raise RuntimeError("K and V must have the same shape")
    kv_model = d_model
    if num_kv_heads is not None:
        num_kv_heads = int(num_kv_heads)
        if num_heads < 1 or d_model % num_heads != 0 or num_kv_heads < 1:
            raise RuntimeError("d_model must be divisible by num_heads, and num_kv_heads positive")
        kv_model = num_kv_heads * (d_model // num_heads)
    if Kc.numel() % kv_model != 0:
        raise RuntimeError("K.numel() must be divisible by d_model" if num_kv_heads is None
                           else "K.numel() must be divisible by num_kv_heads * d")
    Bk, Nk = _shape(Kc, kv_model)
    if Bk != B:
        raise RuntimeError("Q and K must have the same batch count")
    kernel = _known_kernel(kernel)
    out = _out_for(out, Qc, "shape")
    lib = _lib.load()
    with _current_stream(Qc.device) as stream:
        flags = _lib.QMHA_FLAG_CAUSAL if causal else 0
        if num_kv_heads is None:
            st = lib.qmha_solve_rect(Qc.data_ptr(), Kc.data_ptr(), Vc.data_ptr(), out.data_ptr(), B, Nq, Nk, d_model,
                                     num_heads, _lib.variant_id(kernel), flags, None, 0, stream)
        else:
            st = lib.qmha_solve_gqa(Qc.data_ptr(), Kc.data_ptr(), Vc.data_ptr(), out.data_ptr(), B, Nq, Nk, d_model,
                                    num_heads, num_kv_heads, _lib.variant_id(kernel), flags, None, 0, stream)
    _lib.check(st, f"{what}({kernel})")
    return out


class KVCache:
    """A persistent quantised K/V cache (qmha_kv_cache_*; additive, no reference counterpart): chunked prefill and
    decode without re-running the K/V pre-pass over rows an earlier call already quantised / converted.

        cache = KVCache(B, cap, d_model, num_heads)          # fa_tc_int8_b (d = 32 / 64 / 128) or fa_tc_v1a (64 / 128)
        cache.append(K_chunk, V_chunk)                       # [B, n, d_model] (or [n, d_model] for B = 1), n % 32 == 0
        O = cache.attend(Q_chunk)                            # row r attends cache rows j <= r + (len - Nq)

    The object owns a torch.uint8 tensor of qmha_kv_cache_bytes (`.mem`).  append and attend are enqueued on torch's
    current stream; the caller keeps the operations on one cache ordered (one stream, or its own events).
    attend(Q, causal=False) needs a full cache (len == cap): every row attends all cap rows.  truncate(n) drops rows
    from the end (n % 32 == 0, n <= len); nothing is enqueued.  GroupedKVCache (below) is the same cache over fewer
    K/V heads than query heads.
    append_at(K, V, pos) / attend_varlen(Q, lens) take a row / a length per sequence from int32 [B] tensors on the
    device, read by the kernels when they run: sequences of different lengths in one cache, and a step that is captured
    once and replayed while the caller advances pos / lens in device memory.  They leave `len` alone.
    enable_tokens() once, then append_tokens(K, V, pos) / attend_tokens(Q, lens): the same at any length -- a prompt of
    1000 rows, a decode step of one (qmha_kv_cache_append_tokens / qmha_attend_cached_tokens; causal only).
    enable_split(chunk_rows) once, then attend_tokens_split(Q, lens): attend_tokens with the key sweep cut into chunks and
    a combine pass (qmha_attend_cached_tokens_split), for a decode step on long sequences.
    append_packed(K, V, cu, pos, max_n) / attend_packed(Q, cu, lens, max_nq): the token calls with a count per sequence --
    packed [total, ...] operands and an int32 [B + 1] cu on the device, for a step that mixes prefill and decode."""

    def __init__(self, B: int, cap: int, d_model: int, num_heads: int, kernel: str = _lib.DEFAULT_KERNEL, device="cuda"):
        self._setup(B, cap, d_model, num_heads, None, kernel, device)

    def _setup(self, B, cap, d_model, num_heads, num_kv_heads, kernel, device):
        self.B, self.cap, self.d_model, self.num_heads, self.kernel = int(B), int(cap), int(d_model), int(num_heads), kernel
        self.num_kv_heads = self.num_heads if num_kv_heads is None else int(num_kv_heads)
        # row width of K and V (d_model unless grouped; a bad head count is left to the library's checks)
        self.kv_model = self.d_model
        if num_kv_heads is not None and self.num_heads > 0 and self.d_model % self.num_heads == 0:
            self.kv_model = self.num_kv_heads * (self.d_model // self.num_heads)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("KVCache needs a CUDA device")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        lib = _lib.load()
        vid = _lib.variant_id(kernel)
        self._handle = None
        self.tail = None  # enable_tokens()
        self.split_scratch = None  # enable_split()
        if num_kv_heads is None:
            nbytes = lib.qmha_kv_cache_bytes(self.B, self.cap, self.d_model, self.num_heads, vid)
        else:  # the carve of num_kv_heads heads
            nbytes = lib.qmha_kv_cache_bytes(self.B, self.cap, self.kv_model, self.num_kv_heads, vid) if self.num_kv_heads > 0 else 0
        # zero-filled: rows beyond len are never read, but a read-back of the tensor is then reproducible
        self.mem = torch.zeros(max(nbytes, 1), dtype=torch.uint8, device=self.device)
        handle = ctypes.c_void_p()
        if num_kv_heads is None:
            st = lib.qmha_kv_cache_create(ctypes.byref(handle), self.mem.data_ptr(), nbytes, self.B, self.cap, self.d_model,
                                          self.num_heads, vid)
        else:
            st = lib.qmha_kv_cache_create_gqa(ctypes.byref(handle), self.mem.data_ptr(), nbytes, self.B, self.cap,
                                              self.d_model, self.num_heads, self.num_kv_heads, vid)
        _lib.check(st, f"KVCache({kernel})")
        self._handle = handle

    def __del__(self):
        if getattr(self, "_handle", None):
            _lib.load().qmha_kv_cache_destroy(self._handle)
            self._handle = None

    @property
    def len(self) -> int:
        return _lib.load().qmha_kv_cache_len(self._handle)

    def _rows(self, X: torch.Tensor, name: str, width: Optional[int] = None) -> torch.Tensor:
        width = self.d_model if width is None else width
        if not X.is_cuda:
            raise RuntimeError("Inputs must be CUDA tensors")
        if X.dtype != torch.float32:
            raise RuntimeError(f"{name} must be float32")
        if X.device != self.device:
            raise RuntimeError(f"{name} must be on the cache's device {self.device}")
        Xc = X.contiguous()
        if Xc.dim() == 2 and self.B == 1:
            Xc = Xc.unsqueeze(0)
        if Xc.dim() != 3 or Xc.shape[0] != self.B or Xc.shape[2] != width:
            raise RuntimeError(f"{name} must be [B = {self.B}, n, d_model = {width}]"
                               + (" or [n, d_model]" if self.B == 1 else ""))
        return Xc

    def append(self, K: torch.Tensor, V: torch.Tensor) -> None:
        Kc, Vc = self._rows(K, "K", self.kv_model), self._rows(V, "V", self.kv_model)
        if Kc.shape != Vc.shape:
            raise RuntimeError("K and V must have the same shape")
        with _current_stream(self.device) as stream:
            st = _lib.load().qmha_kv_cache_append(self._handle, Kc.data_ptr(), Vc.data_ptr(), Kc.shape[1], stream)
        _lib.check(st, f"KVCache.append({self.kernel})")

    def attend(self, Q: torch.Tensor, causal: bool = True, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        Qc = self._rows(Q, "Q")
        out = _out_for(out, Qc, "size")
        with _current_stream(self.device) as stream:
            st = _lib.load().qmha_attend_cached(self._handle, Qc.data_ptr(), out.data_ptr(), Qc.shape[1],
                                                _lib.QMHA_FLAG_CAUSAL if causal else 0, stream)
        _lib.check(st, f"KVCache.attend({self.kernel})")
        return out.view(Q.shape) if out.numel() == Q.numel() and out.dim() != Q.dim() else out

    def truncate(self, n: int) -> None:
        _lib.check(_lib.load().qmha_kv_cache_truncate(self._handle, int(n)), "KVCache.truncate")

    def _per_seq(self, t: torch.Tensor, name: str) -> torch.Tensor:
        """A per-sequence int32 [B] tensor on the cache's device, read by the kernel when it runs (not by the host)."""
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise RuntimeError(f"{name} must be a CUDA tensor")
        if t.dtype != torch.int32:
            raise RuntimeError(f"{name} must be int32")
        if t.device != self.device:
            raise RuntimeError(f"{name} must be on the cache's device {self.device}")
        if t.dim() != 1 or t.shape[0] != self.B or not t.is_contiguous():
            raise RuntimeError(f"{name} must be a contiguous tensor of shape [B = {self.B}]")
        return t

    def append_at(self, K: torch.Tensor, V: torch.Tensor, pos: torch.Tensor) -> None:
        """append with a row per sequence (qmha_kv_cache_append_at): sequence b's n rows go to cache rows
        [pos[b], pos[b] + n).  pos: int32 [B] on the device, read by the kernel -- the tensor itself, not a copy, so a
        captured call follows later changes of it.  A sequence whose pos[b] is negative, no multiple of 32 or beyond
        cap - n writes nothing.  `len` is neither read nor changed."""
        Kc, Vc = self._rows(K, "K", self.kv_model), self._rows(V, "V", self.kv_model)
        if Kc.shape != Vc.shape:
            raise RuntimeError("K and V must have the same shape")
        pos = self._per_seq(pos, "pos")
        with _current_stream(self.device) as stream:
            st = _lib.load().qmha_kv_cache_append_at(self._handle, Kc.data_ptr(), Vc.data_ptr(), Kc.shape[1], pos.data_ptr(),
                                                     stream)
        _lib.check(st, f"KVCache.append_at({self.kernel})")

    def attend_varlen(self, Q: torch.Tensor, lens: torch.Tensor, causal: bool = True,
                      out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """attend with a length per sequence (qmha_attend_cached_varlen): sequence b attends its first lens[b] cache
        rows -- causal: row r attends rows j <= r + (lens[b] - Nq); causal=False: every row attends rows [0, lens[b]),
        whatever cap is.  lens: int32 [B] on the device, read by the kernel (the tensor itself, as append_at's pos).  A
        sequence whose lens[b] is no multiple of 32, above cap, or below Nq (causal) / 32 (not) gets zeros."""
        Qc = self._rows(Q, "Q")
        lens = self._per_seq(lens, "lens")
        out = _out_for(out, Qc, "size")
        with _current_stream(self.device) as stream:
            st = _lib.load().qmha_attend_cached_varlen(self._handle, Qc.data_ptr(), out.data_ptr(), Qc.shape[1],
                                                       lens.data_ptr(), _lib.QMHA_FLAG_CAUSAL if causal else 0, stream)
        _lib.check(st, f"KVCache.attend_varlen({self.kernel})")
        return out.view(Q.shape) if out.numel() == Q.numel() and out.dim() != Q.dim() else out


    def enable_tokens(self) -> None:
        """Allocate and attach the tail append_tokens needs (qmha_kv_cache_attach_tail): the raw rows of each sequence's
        open 32-row group, `.tail` (int8; an fp16 cache needs none).  Once, and outside a graph capture: append_tokens
        and attend_tokens themselves allocate nothing."""
        if self.tail is not None:
            return
        lib = _lib.load()
        nbytes = lib.qmha_kv_cache_tail_bytes(self._handle)
        self.tail = torch.zeros(max(nbytes, 1), dtype=torch.uint8, device=self.device)
        _lib.check(lib.qmha_kv_cache_attach_tail(self._handle, self.tail.data_ptr(), nbytes), f"KVCache.enable_tokens({self.kernel})")

    def append_tokens(self, K: torch.Tensor, V: torch.Tensor, pos: torch.Tensor) -> None:
        """append_at for any number of rows at any row (qmha_kv_cache_append_tokens): sequence b's n >= 1 rows go to cache
        rows [pos[b], pos[b] + n), and every 32-row group they touch holds what append_at writes for the group's rows so
        far, zero-padded (int8: the open group is quantised again from its raw rows).  A sequence whose pos[b] is
        negative or beyond cap - n writes nothing.  Needs enable_tokens() on an int8 cache."""
        Kc, Vc = self._rows(K, "K", self.kv_model), self._rows(V, "V", self.kv_model)
        if Kc.shape != Vc.shape:
            raise RuntimeError("K and V must have the same shape")
        pos = self._per_seq(pos, "pos")
        with _current_stream(self.device) as stream:
            st = _lib.load().qmha_kv_cache_append_tokens(self._handle, Kc.data_ptr(), Vc.data_ptr(), Kc.shape[1], pos.data_ptr(),
                                                         stream)
        _lib.check(st, f"KVCache.append_tokens({self.kernel})")

    def attend_tokens(self, Q: torch.Tensor, lens: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Causal attend_varlen for any Nq >= 1 and any lengths (qmha_attend_cached_tokens): row r of sequence b attends
        cache rows j <= r + (lens[b] - Nq).  A sequence whose lens[b] is below Nq or above cap gets zeros."""
        Qc = self._rows(Q, "Q")
        lens = self._per_seq(lens, "lens")
        out = _out_for(out, Qc, "size")
        with _current_stream(self.device) as stream:
            st = _lib.load().qmha_attend_cached_tokens(self._handle, Qc.data_ptr(), out.data_ptr(), Qc.shape[1], lens.data_ptr(),
                                                       _lib.QMHA_FLAG_CAUSAL, stream)
        _lib.check(st, f"KVCache.attend_tokens({self.kernel})")
        return out.view(Q.shape) if out.numel() == Q.numel() and out.dim() != Q.dim() else out

    def attend_tokens_window(self, Q: torch.Tensor, lens: torch.Tensor, window: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """attend_tokens under a sliding window (qmha_attend_cached_tokens_window): row r of sequence b attends the cache
        rows j with r + (lens[b] - Nq) - window < j <= r + (lens[b] - Nq), the last min(window, r + lens[b] - Nq + 1) keys.
        window: a multiple of 32, >= 32; window >= cap gives attend_tokens' bits.  Validity rules are attend_tokens'."""
        Qc = self._rows(Q, "Q")
        lens = self._per_seq(lens, "lens")
        out = _out_for(out, Qc, "size")
        with _current_stream(self.device) as stream:
            st = _lib.load().qmha_attend_cached_tokens_window(self._handle, Qc.data_ptr(), out.data_ptr(), Qc.shape[1], lens.data_ptr(),
                                                              int(window), _lib.QMHA_FLAG_CAUSAL, stream)
        _lib.check(st, f"KVCache.attend_tokens_window({self.kernel})")
        return out.view(Q.shape) if out.numel() == Q.numel() and out.dim() != Q.dim() else out

    def enable_split(self, chunk_rows: int, max_nq: int = 32) -> None:
        """Allocate the scratch of the split-KV attend (qmha_attend_split_bytes at Nq = max_nq), `.split_scratch`, for
        chunks of chunk_rows key rows: a multiple of 64 with 64 <= chunk_rows <= cap.  Once (a second call replaces the
        scratch), and outside a graph capture: the split attend itself allocates nothing.  One scratch serves one call
        at a time: calls in flight on different streams need caches, or scratches, of their own."""
        chunk_rows, max_nq = int(chunk_rows), int(max_nq)
        nbytes = _lib.load().qmha_attend_split_bytes(self._handle, max_nq, chunk_rows)
        if nbytes == 0:
            raise RuntimeError(f"enable_split: chunk_rows = {chunk_rows} must be a multiple of 64 with 64 <= chunk_rows <= cap = "
                               f"{self.cap}, and 1 <= max_nq = {max_nq} <= cap")
        self.split_chunk_rows, self.split_max_nq = chunk_rows, max_nq
        self.split_scratch = torch.zeros(nbytes, dtype=torch.uint8, device=self.device)

    def _split_ready(self, Nq: int, what: str) -> None:
        if getattr(self, "split_scratch", None) is None:
            raise RuntimeError(f"{what}: call enable_split(chunk_rows) first")
        if Nq > self.split_max_nq:
            raise RuntimeError(f"{what}: Nq = {Nq} rows exceed enable_split's max_nq = {self.split_max_nq}")

    def split_partials(self, Nq: int):
        """What the last split attend of Nq rows left in `.split_scratch`, as views: (Oc [B, NC, Nq, d_model],
        m [B, NC, Nq, num_heads], l [B, NC, Nq, num_heads]), NC = ceil(cap / chunk_rows) -- each chunk's normalised
        output, running maximum (log2 units) and row sum.  Only the chunks a row reaches are written (include/launchers.h)."""
        Nq = int(Nq)
        self._split_ready(Nq, "split_partials")
        if Nq < 1:
            raise RuntimeError("split_partials: Nq must be at least 1")
        nc = -(-self.cap // self.split_chunk_rows)
        rows, h = self.B * nc * Nq, self.num_heads
        al = lambda x: -(-x // 256) * 256  # noqa: E731 -- each array starts on a multiple of 256 bytes
        o_bytes, s_bytes = 4 * rows * self.d_model, 4 * rows * h
        total = al(o_bytes) + 2 * al(s_bytes)
        if total != _lib.load().qmha_attend_split_bytes(self._handle, Nq, self.split_chunk_rows):
            raise RuntimeError("split_partials: the scratch layout is not the library's")
        mem = self.split_scratch
        Oc = mem[:o_bytes].view(torch.float32).view(self.B, nc, Nq, self.d_model)
        m = mem[al(o_bytes):al(o_bytes) + s_bytes].view(torch.float32).view(self.B, nc, Nq, h)
        l = mem[al(o_bytes) + al(s_bytes):al(o_bytes) + al(s_bytes) + s_bytes].view(torch.float32).view(self.B, nc, Nq, h)
        return Oc, m, l

    def attend_tokens_split(self, Q: torch.Tensor, lens: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """attend_tokens with the key sweep in chunks of enable_split's chunk_rows and a combine pass
        (qmha_attend_cached_tokens_split): for a decode step on long sequences.  Same arguments, validity rules and
        accuracy contract; a deterministic result of its own, not attend_tokens' bits."""
        Qc = self._rows(Q, "Q")
        lens = self._per_seq(lens, "lens")
        self._split_ready(Qc.shape[1], "attend_tokens_split")
        out = _out_for(out, Qc, "size")
        with _current_stream(self.device) as stream:
            st = _lib.load().qmha_attend_cached_tokens_split(self._handle, Qc.data_ptr(), out.data_ptr(), Qc.shape[1], lens.data_ptr(),
                                                             self.split_chunk_rows, self.split_scratch.data_ptr(),
                                                             self.split_scratch.numel(), _lib.QMHA_FLAG_CAUSAL, stream)
        _lib.check(st, f"KVCache.attend_tokens_split({self.kernel})")
        return out.view(Q.shape) if out.numel() == Q.numel() and out.dim() != Q.dim() else out

    def _packed_rows(self, X: torch.Tensor, name: str, width: int) -> torch.Tensor:
        """A packed operand: float32 [total, width] on the cache's device, no batch axis."""
        if not isinstance(X, torch.Tensor) or not X.is_cuda:
            raise RuntimeError("Inputs must be CUDA tensors")
        if X.dtype != torch.float32:
            raise RuntimeError(f"{name} must be float32")
        if X.device != self.device:
            raise RuntimeError(f"{name} must be on the cache's device {self.device}")
        Xc = X.contiguous()
        if Xc.dim() != 2 or Xc.shape[0] < 1 or Xc.shape[1] != width:
            raise RuntimeError(f"{name} must be [total, d_model = {width}] (packed: no batch axis)")
        return Xc

    def _cu(self, t: torch.Tensor) -> torch.Tensor:
        """cu: int32 [B + 1] on the cache's device, read by the kernel when it runs (not by the host)."""
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise RuntimeError("cu must be a CUDA tensor")
        if t.dtype != torch.int32:
            raise RuntimeError("cu must be int32")
        if t.device != self.device:
            raise RuntimeError(f"cu must be on the cache's device {self.device}")
        if t.dim() != 1 or t.shape[0] != self.B + 1 or not t.is_contiguous():
            raise RuntimeError(f"cu must be a contiguous tensor of shape [B + 1 = {self.B + 1}]")
        return t

    def _packed_out(self, out: Optional[torch.Tensor], Qc: torch.Tensor) -> torch.Tensor:
        if out is None:  # zeros: rows outside every range are not written by the call
            return torch.zeros_like(Qc)
        if not out.is_cuda or out.dtype != torch.float32 or out.device != Qc.device or not out.is_contiguous() or out.shape != Qc.shape:
            raise RuntimeError("out must be a contiguous float32 CUDA tensor of Q's shape on Q's device")
        return out

    def append_packed(self, K: torch.Tensor, V: torch.Tensor, cu: torch.Tensor, pos: torch.Tensor, max_n: int) -> None:
        """append_tokens with a row count per sequence (qmha_kv_cache_append_packed): K, V are [total, num_kv_heads * d]
        with no batch axis, sequence b brings the rows [cu[b], cu[b + 1]) to cache rows [pos[b], ...).  cu: int32 [B + 1],
        pos: int32 [B], both on the device and read by the kernel -- the tensors themselves, so a captured call follows
        later changes of them.  max_n: an upper bound of the counts, 1 <= max_n <= min(total, cap).  An empty sequence
        sits out; one with more than max_n rows, a range outside [0, total] or an invalid pos[b] writes nothing."""
        Kc, Vc = self._packed_rows(K, "K", self.kv_model), self._packed_rows(V, "V", self.kv_model)
        if Kc.shape != Vc.shape:
            raise RuntimeError("K and V must have the same shape")
        cu, pos = self._cu(cu), self._per_seq(pos, "pos")
        with _current_stream(self.device) as stream:
            st = _lib.load().qmha_kv_cache_append_packed(self._handle, Kc.data_ptr(), Vc.data_ptr(), Kc.shape[0], int(max_n),
                                                         cu.data_ptr(), pos.data_ptr(), stream)
        _lib.check(st, f"KVCache.append_packed({self.kernel})")

    def attend_packed(self, Q: torch.Tensor, cu: torch.Tensor, lens: torch.Tensor, max_nq: int,
                      out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """attend_tokens with a query count per sequence (qmha_attend_cached_packed): Q is [total, d_model] with no batch
        axis, rows [cu[b], cu[b + 1]) are sequence b's, and each sequence gets the rows attend_tokens writes for a batch
        of its own count.  max_nq: an upper bound of the counts, 1 <= max_nq <= min(total, cap).  An empty sequence sits
        out; one with more than max_nq rows or an invalid lens[b] gets zeros; rows outside every range are not written."""
        Qc = self._packed_rows(Q, "Q", self.d_model)
        cu, lens = self._cu(cu), self._per_seq(lens, "lens")
        out = self._packed_out(out, Qc)
        with _current_stream(self.device) as stream:
            st = _lib.load().qmha_attend_cached_packed(self._handle, Qc.data_ptr(), out.data_ptr(), Qc.shape[0], int(max_nq),
                                                       cu.data_ptr(), lens.data_ptr(), _lib.QMHA_FLAG_CAUSAL, stream)
        _lib.check(st, f"KVCache.attend_packed({self.kernel})")
        return out


class GroupedKVCache(KVCache):
    """KVCache for grouped-query attention (qmha_kv_cache_create_gqa): the cache holds num_kv_heads K/V heads shared
    by the num_heads query heads, append takes [B, n, num_kv_heads * d] (d = d_model / num_heads), attend takes
    [B, Nq, d_model] as before, and `.mem` is num_heads / num_kv_heads times smaller.  num_kv_heads = None is KVCache.
    (A class of its own: KVCache keeps the argument list its callers and tests know.)"""

    def __init__(self, B: int, cap: int, d_model: int, num_heads: int, num_kv_heads: Optional[int] = None,
                 kernel: str = _lib.DEFAULT_KERNEL, device="cuda"):
        self._setup(B, cap, d_model, num_heads, num_kv_heads, kernel, device)


class PagedKVCache:
    """A paged K/V cache (qmha_kv_cache_create_paged): `.mem` is a pool of num_pages pages of page_rows rows of all
    num_kv_heads K/V heads (page_rows % 64 == 0), and an int32 [B, max_pages] block table on the device -- the caller's,
    passed with every call and read by the kernels when they run -- says in which page each page_rows rows of a
    sequence live: row r of sequence b is row r % page_rows of page table[b, r // page_rows].

        cache = PagedKVCache(B, num_pages, page_rows, max_pages, d_model, num_heads)
        cache.enable_tokens()
        cache.append_paged(K, V, pos, table)                 # K, V [B, n, num_kv_heads * d], any n >= 1
        O = cache.attend_paged(Q, lens, table)               # Q [B, Nq, d_model], any Nq >= 1, causal

    The calls are append_tokens / attend_tokens of a contiguous cache with the row looked up, bit for bit.  A sequence
    whose pos / lens is out of range, or that uses a table entry outside [0, num_pages), writes nothing / gets zeros;
    entries behind the pages a call uses are not looked at.  Two sequences may name one page in an attend (a shared
    prefix); two sequences writing one page in one append is the caller's error."""

    def __init__(self, B: int, num_pages: int, page_rows: int, max_pages: int, d_model: int, num_heads: int,
                 num_kv_heads: Optional[int] = None, kernel: str = _lib.DEFAULT_KERNEL, device="cuda"):
        self.B, self.num_pages, self.page_rows, self.max_pages = int(B), int(num_pages), int(page_rows), int(max_pages)
        self.d_model, self.num_heads, self.kernel = int(d_model), int(num_heads), kernel
        self.num_kv_heads = self.num_heads if num_kv_heads is None else int(num_kv_heads)
        self.cap = self.max_pages * self.page_rows  # a sequence's logical capacity
        self.kv_model = self.d_model  # row width of K and V (a bad head count is left to the library's checks)
        if self.num_heads > 0 and self.d_model % self.num_heads == 0:
            self.kv_model = self.num_kv_heads * (self.d_model // self.num_heads)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("PagedKVCache needs a CUDA device")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        lib = _lib.load()
        vid = _lib.variant_id(kernel)
        self._handle = None
        self.tail = None  # enable_tokens()
        self.split_scratch = None  # enable_split()
        nbytes = lib.qmha_kv_cache_paged_bytes(self.num_pages, self.page_rows, self.d_model, self.num_heads, self.num_kv_heads, vid)
        self.mem = torch.zeros(max(nbytes, 1), dtype=torch.uint8, device=self.device)
        handle = ctypes.c_void_p()
        st = lib.qmha_kv_cache_create_paged(ctypes.byref(handle), self.mem.data_ptr(), nbytes, self.B, self.num_pages, self.page_rows,
                                            self.max_pages, self.d_model, self.num_heads, self.num_kv_heads, vid)
        _lib.check(st, f"PagedKVCache({kernel})")
        self._handle = handle

    __del__ = KVCache.__del__
    _rows = KVCache._rows
    _per_seq = KVCache._per_seq
    enable_tokens = KVCache.enable_tokens
    enable_split = KVCache.enable_split
    _split_ready = KVCache._split_ready
    split_partials = KVCache.split_partials

    def _table(self, t: torch.Tensor) -> torch.Tensor:
        """The block table: int32 [B, max_pages] on the cache's device, read by the kernel when it runs (not by the host)."""
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise RuntimeError("table must be a CUDA tensor")
        if t.dtype != torch.int32:
            raise RuntimeError("table must be int32")
        if t.device != self.device:
            raise RuntimeError(f"table must be on the cache's device {self.device}")
        if t.dim() != 2 or tuple(t.shape) != (self.B, self.max_pages) or not t.is_contiguous():
            raise RuntimeError(f"table must be a contiguous tensor of shape [B = {self.B}, max_pages = {self.max_pages}]")
        return t

    def append_paged(self, K: torch.Tensor, V: torch.Tensor, pos: torch.Tensor, table: torch.Tensor) -> None:
        """append_tokens through the table (qmha_kv_cache_append_paged): sequence b's n >= 1 rows go to logical rows
        [pos[b], pos[b] + n).  pos: int32 [B], table: int32 [B, max_pages], both on the device and read by the kernel --
        the tensors themselves, so a captured call follows later changes of them.  A sequence whose pos[b] is negative
        or beyond cap - n, or whose touched pages have an entry outside [0, num_pages), writes nothing.  Needs
        enable_tokens() on an int8 cache."""
        Kc, Vc = self._rows(K, "K", self.kv_model), self._rows(V, "V", self.kv_model)
        if Kc.shape != Vc.shape:
            raise RuntimeError("K and V must have the same shape")
        pos, table = self._per_seq(pos, "pos"), self._table(table)
        with _current_stream(self.device) as stream:
            st = _lib.load().qmha_kv_cache_append_paged(self._handle, Kc.data_ptr(), Vc.data_ptr(), Kc.shape[1], pos.data_ptr(),
                                                        table.data_ptr(), stream)
        _lib.check(st, f"PagedKVCache.append_paged({self.kernel})")

    def attend_paged(self, Q: torch.Tensor, lens: torch.Tensor, table: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """attend_tokens through the table (qmha_attend_cached_paged): row r of sequence b attends its logical rows
        j <= r + (lens[b] - Nq).  A sequence whose lens[b] is below Nq or above cap, or whose used pages have an entry
        outside [0, num_pages), gets zeros."""
        Qc = self._rows(Q, "Q")
        lens, table = self._per_seq(lens, "lens"), self._table(table)
        out = _out_for(out, Qc, "size")
        with _current_stream(self.device) as stream:
            st = _lib.load().qmha_attend_cached_paged(self._handle, Qc.data_ptr(), out.data_ptr(), Qc.shape[1], lens.data_ptr(),
                                                      table.data_ptr(), _lib.QMHA_FLAG_CAUSAL, stream)
        _lib.check(st, f"PagedKVCache.attend_paged({self.kernel})")
        return out.view(Q.shape) if out.numel() == Q.numel() and out.dim() != Q.dim() else out

    def attend_paged_window(self, Q: torch.Tensor, lens: torch.Tensor, table: torch.Tensor, window: int,
                            out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """attend_tokens_window through the table (qmha_attend_cached_paged_window), bit for bit.  Only the table columns
        whose pages hold rows of the window (widened to its first two-tile stage) are read: columns behind them may hold
        anything, and their pages may belong to another sequence.  A used entry outside [0, num_pages) gives zeros."""
        Qc = self._rows(Q, "Q")
        lens, table = self._per_seq(lens, "lens"), self._table(table)
        out = _out_for(out, Qc, "size")
        with _current_stream(self.device) as stream:
            st = _lib.load().qmha_attend_cached_paged_window(self._handle, Qc.data_ptr(), out.data_ptr(), Qc.shape[1], lens.data_ptr(),
                                                             table.data_ptr(), int(window), _lib.QMHA_FLAG_CAUSAL, stream)
        _lib.check(st, f"PagedKVCache.attend_paged_window({self.kernel})")
        return out.view(Q.shape) if out.numel() == Q.numel() and out.dim() != Q.dim() else out

    def attend_paged_split(self, Q: torch.Tensor, lens: torch.Tensor, table: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """attend_tokens_split through the table (qmha_attend_cached_paged_split), bit for bit; needs enable_split()."""
        Qc = self._rows(Q, "Q")
        lens, table = self._per_seq(lens, "lens"), self._table(table)
        self._split_ready(Qc.shape[1], "attend_paged_split")
        out = _out_for(out, Qc, "size")
        with _current_stream(self.device) as stream:
            st = _lib.load().qmha_attend_cached_paged_split(self._handle, Qc.data_ptr(), out.data_ptr(), Qc.shape[1], lens.data_ptr(),
                                                            table.data_ptr(), self.split_chunk_rows, self.split_scratch.data_ptr(),
                                                            self.split_scratch.numel(), _lib.QMHA_FLAG_CAUSAL, stream)
        _lib.check(st, f"PagedKVCache.attend_paged_split({self.kernel})")
        return out.view(Q.shape) if out.numel() == Q.numel() and out.dim() != Q.dim() else out

    _packed_rows = KVCache._packed_rows
    _cu = KVCache._cu
    _packed_out = KVCache._packed_out

    def append_paged_packed(self, K: torch.Tensor, V: torch.Tensor, cu: torch.Tensor, pos: torch.Tensor, table: torch.Tensor,
                            max_n: int) -> None:
        """append_packed through the table (qmha_kv_cache_append_paged_packed): K, V [total, num_kv_heads * d], sequence
        b's rows [cu[b], cu[b + 1]) go to its logical rows [pos[b], ...); append_paged's rules per sequence."""
        Kc, Vc = self._packed_rows(K, "K", self.kv_model), self._packed_rows(V, "V", self.kv_model)
        if Kc.shape != Vc.shape:
            raise RuntimeError("K and V must have the same shape")
        cu, pos, table = self._cu(cu), self._per_seq(pos, "pos"), self._table(table)
        with _current_stream(self.device) as stream:
            st = _lib.load().qmha_kv_cache_append_paged_packed(self._handle, Kc.data_ptr(), Vc.data_ptr(), Kc.shape[0], int(max_n),
                                                               cu.data_ptr(), pos.data_ptr(), table.data_ptr(), stream)
        _lib.check(st, f"PagedKVCache.append_paged_packed({self.kernel})")

    def attend_paged_packed(self, Q: torch.Tensor, cu: torch.Tensor, lens: torch.Tensor, table: torch.Tensor, max_nq: int,
                            out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """attend_packed through the table (qmha_attend_cached_paged_packed): Q [total, d_model], rows [cu[b], cu[b + 1])
        are sequence b's; attend_paged's rules per sequence."""
        Qc = self._packed_rows(Q, "Q", self.d_model)
        cu, lens, table = self._cu(cu), self._per_seq(lens, "lens"), self._table(table)
        out = self._packed_out(out, Qc)
        with _current_stream(self.device) as stream:
            st = _lib.load().qmha_attend_cached_paged_packed(self._handle, Qc.data_ptr(), out.data_ptr(), Qc.shape[0], int(max_nq),
                                                             cu.data_ptr(), lens.data_ptr(), table.data_ptr(), _lib.QMHA_FLAG_CAUSAL,
                                                             stream)
        _lib.check(st, f"PagedKVCache.attend_paged_packed({self.kernel})")
        return out


def quantize_int8(X: torch.Tensor, d_model: int, num_heads: int, layout: int = 0):
    """The INT8 pre-pass as an op: per-32-row-group symmetric int8 of every head.

    Returns (Xi [B, h, N, d] int8 (layout 0) or [B, h, N/32, d, 32] (layout 1, V operand
    order), scales [B, h, N/32] fp32); layout 2: [B, h, N, d] rows with one scale per head slice
    (the fa_tc_int8_pt per-tensor mode), scales [B, h]."""
    if not X.is_cuda or X.dtype != torch.float32:
        raise RuntimeError("X must be a float32 CUDA tensor")
    Xc = X.contiguous()
    B, N = _shape(Xc, d_model)
    d = d_model // num_heads
    if layout in (0, 2):
        Xi = torch.empty((B, num_heads, N, d), dtype=torch.int8, device=X.device)
    else:
        Xi = torch.empty((B, num_heads, N // 32, d, 32), dtype=torch.int8, device=X.device)
    sc = torch.empty((B, num_heads) if layout == 2 else (B, num_heads, N // 32), dtype=torch.float32, device=X.device)
    with _current_stream(Xc.device) as stream:
        st = _lib.load().qmha_quantize_int8(Xc.data_ptr(), B, N, d_model, num_heads, Xi.data_ptr(), sc.data_ptr(),
                                            layout, stream)
    _lib.check(st, "quantize_int8")
    return Xi, sc


def debug_qk_int32(Q: torch.Tensor, K: torch.Tensor, d_model: int, num_heads: int, head: int) -> torch.Tensor:
    """int32 S = Q_i8 K_i8^T of one head through the INT8 path's MFMA operand path (test hook)."""
    if not (Q.is_cuda and K.is_cuda):
        raise RuntimeError("Inputs must be CUDA tensors")
    Qc, Kc = Q.contiguous(), K.contiguous()
    N = Qc.numel() // d_model
    S = torch.empty((N, N), dtype=torch.int32, device=Q.device)
    torch.cuda.synchronize(Q.device)
    with torch.cuda.device(Qc.device):
        st = _lib.load().qmha_debug_qk_int32(Qc.data_ptr(), Kc.data_ptr(), N, d_model, num_heads, head, S.data_ptr())
    _lib.check(st, "debug_qk_int32")
    return S


def debug_fa_int8_dump(Q: torch.Tensor, K: torch.Tensor, V: torch.Tensor, d_model: int, num_heads: int,
                       per_tensor: bool = False):
    """Run the production int8 kernel with its FL_DUMP stores (test hook): returns (O, S, Qi, sQ)
    with O as flash_solve computes it, S [B, h, N, N] int32 = the kernel's own Q@K^T
    accumulators (bias removed), Qi [B, h, N, d] its in-register int8 Q operand, sQ [B, h, N/32].
    per_tensor: the fa_tc_int8_pt kernel instead (sQ then repeats the head slice's one scale)."""
    if not (Q.is_cuda and K.is_cuda and V.is_cuda):
        raise RuntimeError("Inputs must be CUDA tensors")
    Qc, Kc, Vc = Q.contiguous(), K.contiguous(), V.contiguous()
    B, N = _shape(Qc, d_model)
    d = d_model // num_heads
    O = torch.empty_like(Qc)
    S = torch.empty((B, num_heads, N, N), dtype=torch.int32, device=Q.device)
    Qi = torch.empty((B, num_heads, N, d), dtype=torch.int8, device=Q.device)
    sQ = torch.empty((B, num_heads, N // 32), dtype=torch.float32, device=Q.device)
    torch.cuda.synchronize(Q.device)
    with torch.cuda.device(Qc.device):
        lib = _lib.load()
        fn = lib.qmha_debug_fa_int8_pt_dump if per_tensor else lib.qmha_debug_fa_int8_dump
        st = fn(Qc.data_ptr(), Kc.data_ptr(), Vc.data_ptr(), O.data_ptr(), B, N, d_model, num_heads, S.data_ptr(),
                Qi.data_ptr(), sQ.data_ptr())
    _lib.check(st, "debug_fa_int8_dump")
    return O, S, Qi, sQ


# What debug_fa_int8_pstage pre-fills its buffers with: values no kernel writes there (|S| < 2^22, |T| < 2^20 or
# INT32_MIN, Pi in 0..127 or -128, Qi never -128 from a symmetric scale, sQ / sP / l >= 0, m >= m0 = 0).
PSTAGE_SENTINEL = {"S": 0x7FFFFFF1, "Qi": -128, "sQ": -3.0e38, "m": -3.0e38, "sP": -3.0e38, "Pi": -127, "T": 0x7FFFFFF1,
                   "l": -3.0e38}


def debug_fa_int8_pstage(Q: torch.Tensor, K: torch.Tensor, V: torch.Tensor, d_model: int, num_heads: int,
                         causal: bool = False):
    """The P stage of fa_tc_int8_b, tile by tile (test hook; qmha_debug_fa_int8_pstage in include/launchers.h).

    Q [B, Nq, d_model], K and V [B, Nk, d_model]: runs the dumping twin of the kernel flash_solve / flash_solve_rect
    would launch and returns (O, dump) with dump a dict of tensors, every one pre-filled with PSTAGE_SENTINEL so
    that what the kernel did not write can be told: S [B, h, Nq, Nk] int32, Qi [B, h, Nq, d] int8, sQ [B, h, Gq],
    m [B, h, Nq, Gk], sP [B, h, Gq, Gk], Pi [B, h, Nq, Nk] int8, T [B, h, Gk, Nq, d] int32, l [B, h, Nq]."""
    if not (Q.is_cuda and K.is_cuda and V.is_cuda):
        raise RuntimeError("Inputs must be CUDA tensors")
    Qc, Kc, Vc = Q.contiguous(), K.contiguous(), V.contiguous()
    B, Nq = _shape(Qc, d_model)
    _, Nk = _shape(Kc, d_model)
    h, d, Gq, Gk = num_heads, d_model // num_heads, Nq // 32, Nk // 32
    O = torch.empty_like(Qc)
    i32, i8, f32 = torch.int32, torch.int8, torch.float32
    shapes = {"S": ((B, h, Nq, Nk), i32), "Qi": ((B, h, Nq, d), i8), "sQ": ((B, h, Gq), f32), "m": ((B, h, Nq, Gk), f32),
              "sP": ((B, h, Gq, Gk), f32), "Pi": ((B, h, Nq, Nk), i8), "T": ((B, h, Gk, Nq, d), i32), "l": ((B, h, Nq), f32)}
    dump = {k: torch.full(shape, PSTAGE_SENTINEL[k], dtype=dt, device=Q.device) for k, (shape, dt) in shapes.items()}
    torch.cuda.synchronize(Q.device)
    with torch.cuda.device(Qc.device):
        st = _lib.load().qmha_debug_fa_int8_pstage(Qc.data_ptr(), Kc.data_ptr(), Vc.data_ptr(), O.data_ptr(), B, Nq, Nk, d_model,
                                                   h, _lib.QMHA_FLAG_CAUSAL if causal else 0,
                                                   *(dump[k].data_ptr() for k in ("S", "Qi", "sQ", "m", "sP", "Pi", "T", "l")))
    _lib.check(st, "debug_fa_int8_pstage")
    return O, dump
