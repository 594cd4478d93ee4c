"""PyTorch custom operator for the MI355X forward kernel (SURVEY.md §8(f)
rank 3: the wrapper that puts the kernel beside PyTorch SDPA on one box).

    import fa_mi355x.torch_op  # registers torch.ops.fa_mi355x.fwd
    o = torch.ops.fa_mi355x.fwd(q, k, v, causal=True)
    o = torch.ops.fa_mi355x.decode(q, k_cache, v_cache, kv_lens, causal=True)
    o = torch.ops.fa_mi355x.decode_paged(q, k_pages, v_pages, block_table, kv_lens, causal=True)
    o = torch.ops.fa_mi355x.decode(q, k8_cache, v8_cache, kv_lens, k_scale=ks, v_scale=vs)  # FP8 cache
    torch.ops.fa_mi355x.cache_append(k_new, v_new, k_cache, v_cache, kv_lens)  # writes the caches
    torch.ops.fa_mi355x.cache_append_paged(k_new, v_new, k_pages, v_pages, block_table, kv_lens)
    o = torch.ops.fa_mi355x.prefill(q, k_cache, v_cache, kv_lens, q_lens, causal=True)  # any Sq
    o = torch.ops.fa_mi355x.prefill_paged(q, k_pages, v_pages, block_table, kv_lens, q_lens)
    o = torch.ops.fa_mi355x.prefill_varlen(q_packed, k_cache, v_cache, cu_seqlens_q, kv_lens)  # [T,Hq,D]
    o = torch.ops.fa_mi355x.prefill_varlen_paged(q_packed, k_pages, v_pages, block_table, cu_seqlens_q, kv_lens)
    torch.ops.fa_mi355x.cache_append_varlen(k_packed, v_packed, k_cache, v_cache, cu_seqlens, kv_lens)
    torch.ops.fa_mi355x.cache_append_varlen_paged(k_packed, v_packed, k_pages, v_pages, block_table, cu_seqlens, kv_lens)
    q_rot = torch.ops.fa_mi355x.rope_append(q, k_new, v_new, k_cache, v_cache, kv_lens, cos, sin)  # RoPE + append
    (and rope_append_paged, rope_append_varlen, rope_append_varlen_paged)
    o = torch.ops.fa_mi355x.attn_varlen(q, k, v, cu_seqlens_q, cu_seqlens_k, causal=False)  # [T,H,D], no cache
    o = torch.ops.fa_mi355x.attn_bshd(q, k, v, causal=True)  # [B,S,H,D], no cache
    dq, dk, dv = torch.ops.fa_mi355x.attn_varlen_bwd(dout, q, k, v, out, lse, cu_seqlens_q, cu_seqlens_k)
    dq, dk, dv, dsinks = torch.ops.fa_mi355x.attn_varlen_bwd(dout, q, k, v, out, lse, cu_seqlens_q, cu_seqlens_k,
                                                             True, window, sinks)  # the .sinks overload
    o = fa_mi355x.flash_attn_varlen_func(q, k, v, cu_seqlens_q)  # differentiable (torch.autograd)
    o = fa_mi355x.flash_attn_varlen_func(q, k, v, cu_seqlens_q, causal=True, window=128, sinks=sinks)

``q, k, v``: fp16 or bf16 ``[B, H, S, D]`` (D = 128 or 64) tensors on the GPU (BHSD, the
reference layout, flash_attention.cu:119-122); returns a new tensor of the same shape and dtype.
The schema is defined with ``torch.library.Library`` and the kernel registered
for the CUDA dispatch key directly (``custom_op``'s extra dispatch layers cost
3.7 us more per call than this registration, 12.2 vs 8.5 us host time on a
short launch, tools/host_overhead.py); a fake (meta) implementation supplies
the output shape, so the op is opaque to ``torch.compile``, and it launches on
the current HIP stream, so it can be captured in a HIP graph.  It calls the
same C ABI as every other entry point; there is no CPU or eager fallback (a
CPU tensor raises ValueError).  Forward only: the Autograd key falls through
(no Python frame on the call path) and the GPU and fake kernels raise when a
gradient would be needed (q, k or v requiring grad with grad mode on)
instead of returning an output that backward would silently ignore.  The
exception is the attention with no cache: flash_attn_varlen_func and
flash_attn_func at the end of this module are torch.autograd.Functions over
the attn_varlen_fwd / attn_varlen_bwd (attn_bshd_fwd / attn_bshd_bwd) ops.
"""
from __future__ import annotations

import torch

from . import (flash_attention_cache_append, flash_attention_cache_append_paged,
               flash_attention_cache_append_varlen, flash_attention_cache_append_varlen_paged,
               flash_attention_bshd, flash_attention_bshd_backward, flash_attention_decode, flash_attention_decode_paged,
               flash_attention_fwd,
               flash_attention_prefill, flash_attention_prefill_paged,
               flash_attention_prefill_varlen, flash_attention_prefill_varlen_paged,
               flash_attention_rope_append, flash_attention_rope_append_paged,
               flash_attention_rope_append_varlen, flash_attention_rope_append_varlen_paged,
               flash_attention_varlen, flash_attention_varlen_backward)
from . import FlashAttentionError, _token_stride

OP_NAME = "fa_mi355x::fwd"

_LIB = torch.library.Library("fa_mi355x", "DEF")
_LIB.define("fwd(Tensor q, Tensor k, Tensor v, bool causal=False) -> Tensor")


def _no_grad_needed(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor) -> None:
    if torch.is_grad_enabled() and (q.requires_grad or k.requires_grad or v.requires_grad):
        raise RuntimeError("fa_mi355x::fwd is forward-only (no backward): call it under "
                           "torch.no_grad() / inference_mode or on tensors that do not require grad")


def _fwd_gpu(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, causal: bool = False) -> torch.Tensor:
    _no_grad_needed(q, k, v)
    return flash_attention_fwd(q.contiguous(), k.contiguous(), v.contiguous(), causal=causal)


def _fwd_cpu(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, causal: bool = False) -> torch.Tensor:
    raise ValueError("fa_mi355x::fwd needs GPU tensors (no CPU path)")


def _fwd_fake(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, causal: bool = False) -> torch.Tensor:
    _no_grad_needed(q, k, v)
    torch._check(q.dim() == 4 and q.shape[-1] in (64, 128), lambda: "expected [B, H, S, 64|128]")
    torch._check(q.dtype in (torch.float16, torch.bfloat16), lambda: "expected fp16 or bf16")
    return torch.empty_like(q, memory_format=torch.contiguous_format)


_LIB.impl("fwd", _fwd_gpu, "CUDA")
_LIB.impl("fwd", torch.library.fallthrough_kernel, "Autograd")
_LIB.impl("fwd", _fwd_cpu, "CPU")
torch.library.register_fake(OP_NAME, _fwd_fake, lib=_LIB)

fwd = torch.ops.fa_mi355x.fwd

# decode(q [B,Hq,Sq,D], k_cache / v_cache [B,Hkv,cap,D], kv_lens int32 [B] or
# None): fa_mi355x.flash_attention_decode behind the same kind of registration.
# k_cache and v_cache must be contiguous (FlashAttentionError otherwise).
# An FP8 cache (both torch.float8_e4m3fn) takes k_scale / v_scale, float32
# [Hkv] or None (= 1.0); their values are read on the device.
DECODE_OP_NAME = "fa_mi355x::decode"
_LIB.define("decode(Tensor q, Tensor k_cache, Tensor v_cache, Tensor? kv_lens=None, "
            "bool causal=True, Tensor? k_scale=None, Tensor? v_scale=None) -> Tensor")


def _decode_gpu(q, k_cache, v_cache, kv_lens=None, causal: bool = True, k_scale=None,
                v_scale=None) -> torch.Tensor:
    _no_grad_needed(q, k_cache, v_cache)
    # the caches are taken as they are: a strided view (a slice of a larger
    # cache) raises instead of being copied, which would move the whole cache
    # once more than the kernel does
    return flash_attention_decode(q.contiguous(), k_cache, v_cache,
                                  None if kv_lens is None else kv_lens.contiguous(), causal=causal,
                                  k_scale=k_scale, v_scale=v_scale)


def _decode_cpu(q, k_cache, v_cache, kv_lens=None, causal: bool = True, k_scale=None,
                v_scale=None) -> torch.Tensor:
    raise ValueError("fa_mi355x::decode needs GPU tensors (no CPU path)")


def _decode_fake(q, k_cache, v_cache, kv_lens=None, causal: bool = True, k_scale=None,
                 v_scale=None) -> torch.Tensor:
    _no_grad_needed(q, k_cache, v_cache)
    torch._check(q.dim() == 4 and q.shape[-1] in (64, 128), lambda: "expected [B, Hq, Sq, 64|128]")
    torch._check(q.dtype in (torch.float16, torch.bfloat16), lambda: "expected fp16 or bf16")
    return torch.empty_like(q, memory_format=torch.contiguous_format)


_LIB.impl("decode", _decode_gpu, "CUDA")
_LIB.impl("decode", torch.library.fallthrough_kernel, "Autograd")
_LIB.impl("decode", _decode_cpu, "CPU")
torch.library.register_fake(DECODE_OP_NAME, _decode_fake, lib=_LIB)

decode = torch.ops.fa_mi355x.decode

# decode_paged(q [B,Hq,Sq,D], k_pages / v_pages [num_pages,Hkv,page_size,D],
# block_table int32 [B,max_pages], kv_lens int32 [B] or None):
# fa_mi355x.flash_attention_decode_paged behind the same kind of registration.
# The pools are taken as they are (a strided pool raises).
DECODE_PAGED_OP_NAME = "fa_mi355x::decode_paged"
_LIB.define("decode_paged(Tensor q, Tensor k_pages, Tensor v_pages, Tensor block_table, "
            "Tensor? kv_lens=None, bool causal=True) -> Tensor")


def _decode_paged_gpu(q, k_pages, v_pages, block_table, kv_lens=None, causal: bool = True,
                      k_scale=None, v_scale=None) -> torch.Tensor:
    _no_grad_needed(q, k_pages, v_pages)
    return flash_attention_decode_paged(q.contiguous(), k_pages, v_pages, block_table.contiguous(),
                                        None if kv_lens is None else kv_lens.contiguous(),
                                        causal=causal, k_scale=k_scale, v_scale=v_scale)


def _decode_paged_cpu(q, k_pages, v_pages, block_table, kv_lens=None, causal: bool = True,
                      k_scale=None, v_scale=None) -> torch.Tensor:
    raise ValueError("fa_mi355x::decode_paged needs GPU tensors (no CPU path)")


def _decode_paged_fake(q, k_pages, v_pages, block_table, kv_lens=None, causal: bool = True,
                       k_scale=None, v_scale=None) -> torch.Tensor:
    _no_grad_needed(q, k_pages, v_pages)
    torch._check(q.dim() == 4 and q.shape[-1] in (64, 128), lambda: "expected [B, Hq, Sq, 64|128]")
    torch._check(q.dtype in (torch.float16, torch.bfloat16), lambda: "expected fp16 or bf16")
    torch._check(block_table.dim() == 2, lambda: "expected a [B, max_pages_per_seq] block table")
    return torch.empty_like(q, memory_format=torch.contiguous_format)


_LIB.impl("decode_paged", _decode_paged_gpu, "CUDA")
_LIB.impl("decode_paged", torch.library.fallthrough_kernel, "Autograd")
_LIB.impl("decode_paged", _decode_paged_cpu, "CPU")
torch.library.register_fake(DECODE_PAGED_OP_NAME, _decode_paged_fake, lib=_LIB)

# The FP8 pool's scales: the default overload's schema is pinned as it stands
# (it takes FP8 pools too, with scales of 1.0), so k_scale / v_scale come in a
# second overload with the same leading arguments.  A call through the packet
# torch.ops.fa_mi355x.decode_paged(...) that names or passes a scale resolves
# to it; every call the default overload accepts still resolves to the default.
DECODE_PAGED_KV8_OP_NAME = "fa_mi355x::decode_paged.kv8"
_LIB.define("decode_paged.kv8(Tensor q, Tensor k_pages, Tensor v_pages, Tensor block_table, "
            "Tensor? kv_lens=None, bool causal=True, Tensor? k_scale=None, "
            "Tensor? v_scale=None) -> Tensor")
_LIB.impl("decode_paged.kv8", _decode_paged_gpu, "CUDA")
_LIB.impl("decode_paged.kv8", torch.library.fallthrough_kernel, "Autograd")
_LIB.impl("decode_paged.kv8", _decode_paged_cpu, "CPU")
torch.library.register_fake(DECODE_PAGED_KV8_OP_NAME, _decode_paged_fake, lib=_LIB)

decode_paged = torch.ops.fa_mi355x.decode_paged

# cache_append(k_new / v_new [B,Hkv,Sn,D], k_cache / v_cache [B,Hkv,cap,D],
# kv_lens int32 [B]: the lengths after the append) and cache_append_paged (the
# pools and the block table): fa_mi355x.flash_attention_cache_append[_paged]
# behind the same kind of registration.  The caches are mutated in place and
# nothing is returned; they are taken as they are (a strided cache raises).
CACHE_APPEND_OP_NAME = "fa_mi355x::cache_append"
_LIB.define("cache_append(Tensor k_new, Tensor v_new, Tensor(a!) k_cache, Tensor(b!) v_cache, "
            "Tensor kv_lens, Tensor? new_lens=None, Tensor? k_scale=None, "
            "Tensor? v_scale=None) -> ()")


def _cache_append_gpu(k_new, v_new, k_cache, v_cache, kv_lens, new_lens=None, k_scale=None,
                      v_scale=None) -> None:
    flash_attention_cache_append(k_new.contiguous(), v_new.contiguous(), k_cache, v_cache,
                                 kv_lens.contiguous(),
                                 None if new_lens is None else new_lens.contiguous(),
                                 k_scale=k_scale, v_scale=v_scale)


def _cache_append_cpu(k_new, v_new, k_cache, v_cache, kv_lens, new_lens=None, k_scale=None,
                      v_scale=None) -> None:
    raise ValueError("fa_mi355x::cache_append needs GPU tensors (no CPU path)")


def _cache_append_fake(k_new, v_new, k_cache, v_cache, kv_lens, new_lens=None, k_scale=None,
                       v_scale=None) -> None:
    torch._check(k_new.dim() == 4 and k_new.shape[-1] in (64, 128), lambda: "expected [B, Hkv, Sn, 64|128]")
    torch._check(k_new.dtype in (torch.float16, torch.bfloat16), lambda: "expected fp16 or bf16")
    torch._check(k_cache.dim() == 4 and v_cache.dim() == 4, lambda: "expected 4-D caches")


_LIB.impl("cache_append", _cache_append_gpu, "CUDA")
_LIB.impl("cache_append", _cache_append_cpu, "CPU")
torch.library.register_fake(CACHE_APPEND_OP_NAME, _cache_append_fake, lib=_LIB)

cache_append = torch.ops.fa_mi355x.cache_append

CACHE_APPEND_PAGED_OP_NAME = "fa_mi355x::cache_append_paged"
_LIB.define("cache_append_paged(Tensor k_new, Tensor v_new, Tensor(a!) k_pages, Tensor(b!) v_pages, "
            "Tensor block_table, Tensor kv_lens, Tensor? new_lens=None, Tensor? k_scale=None, "
            "Tensor? v_scale=None) -> ()")


def _cache_append_paged_gpu(k_new, v_new, k_pages, v_pages, block_table, kv_lens, new_lens=None,
                            k_scale=None, v_scale=None) -> None:
    flash_attention_cache_append_paged(k_new.contiguous(), v_new.contiguous(), k_pages, v_pages,
                                       block_table.contiguous(), kv_lens.contiguous(),
                                       None if new_lens is None else new_lens.contiguous(),
                                       k_scale=k_scale, v_scale=v_scale)


def _cache_append_paged_cpu(k_new, v_new, k_pages, v_pages, block_table, kv_lens, new_lens=None,
                            k_scale=None, v_scale=None) -> None:
    raise ValueError("fa_mi355x::cache_append_paged needs GPU tensors (no CPU path)")


def _cache_append_paged_fake(k_new, v_new, k_pages, v_pages, block_table, kv_lens, new_lens=None,
                             k_scale=None, v_scale=None) -> None:
    _cache_append_fake(k_new, v_new, k_pages, v_pages, kv_lens, new_lens, k_scale, v_scale)
    torch._check(block_table.dim() == 2, lambda: "expected a [B, max_pages_per_seq] block table")


_LIB.impl("cache_append_paged", _cache_append_paged_gpu, "CUDA")
_LIB.impl("cache_append_paged", _cache_append_paged_cpu, "CPU")
torch.library.register_fake(CACHE_APPEND_PAGED_OP_NAME, _cache_append_paged_fake, lib=_LIB)

cache_append_paged = torch.ops.fa_mi355x.cache_append_paged

# prefill(q [B,Hq,Sq,D] of any Sq, k_cache / v_cache [B,Hkv,cap,D], kv_lens and
# q_lens int32 [B] or None) and prefill_paged (the pools and the block table):
# fa_mi355x.flash_attention_prefill[_paged] behind the same kind of
# registration as decode.  The caches are taken as they are (a strided cache
# raises); an FP8 cache takes k_scale / v_scale.  Rows past q_lens of the
# returned tensor are unspecified.
PREFILL_OP_NAME = "fa_mi355x::prefill"
_LIB.define("prefill(Tensor q, Tensor k_cache, Tensor v_cache, Tensor? kv_lens=None, "
            "Tensor? q_lens=None, bool causal=True, Tensor? k_scale=None, "
            "Tensor? v_scale=None) -> Tensor")


def _prefill_gpu(q, k_cache, v_cache, kv_lens=None, q_lens=None, causal: bool = True, k_scale=None,
                 v_scale=None) -> torch.Tensor:
    _no_grad_needed(q, k_cache, v_cache)
    return flash_attention_prefill(q.contiguous(), k_cache, v_cache,
                                   None if kv_lens is None else kv_lens.contiguous(),
                                   None if q_lens is None else q_lens.contiguous(), causal=causal,
                                   k_scale=k_scale, v_scale=v_scale)


def _prefill_cpu(q, k_cache, v_cache, kv_lens=None, q_lens=None, causal: bool = True, k_scale=None,
                 v_scale=None) -> torch.Tensor:
    raise ValueError("fa_mi355x::prefill needs GPU tensors (no CPU path)")


def _prefill_fake(q, k_cache, v_cache, kv_lens=None, q_lens=None, causal: bool = True, k_scale=None,
                  v_scale=None) -> torch.Tensor:
    _no_grad_needed(q, k_cache, v_cache)
    torch._check(q.dim() == 4 and q.shape[-1] in (64, 128), lambda: "expected [B, Hq, Sq, 64|128]")
    torch._check(q.dtype in (torch.float16, torch.bfloat16), lambda: "expected fp16 or bf16")
    return torch.empty_like(q, memory_format=torch.contiguous_format)


_LIB.impl("prefill", _prefill_gpu, "CUDA")
_LIB.impl("prefill", torch.library.fallthrough_kernel, "Autograd")
_LIB.impl("prefill", _prefill_cpu, "CPU")
torch.library.register_fake(PREFILL_OP_NAME, _prefill_fake, lib=_LIB)

prefill = torch.ops.fa_mi355x.prefill

PREFILL_PAGED_OP_NAME = "fa_mi355x::prefill_paged"
_LIB.define("prefill_paged(Tensor q, Tensor k_pages, Tensor v_pages, Tensor block_table, "
            "Tensor? kv_lens=None, Tensor? q_lens=None, bool causal=True, Tensor? k_scale=None, "
            "Tensor? v_scale=None) -> Tensor")


def _prefill_paged_gpu(q, k_pages, v_pages, block_table, kv_lens=None, q_lens=None, causal: bool = True,
                       k_scale=None, v_scale=None) -> torch.Tensor:
    _no_grad_needed(q, k_pages, v_pages)
    return flash_attention_prefill_paged(q.contiguous(), k_pages, v_pages, block_table.contiguous(),
                                         None if kv_lens is None else kv_lens.contiguous(),
                                         None if q_lens is None else q_lens.contiguous(),
                                         causal=causal, k_scale=k_scale, v_scale=v_scale)


def _prefill_paged_cpu(q, k_pages, v_pages, block_table, kv_lens=None, q_lens=None, causal: bool = True,
                       k_scale=None, v_scale=None) -> torch.Tensor:
    raise ValueError("fa_mi355x::prefill_paged needs GPU tensors (no CPU path)")


def _prefill_paged_fake(q, k_pages, v_pages, block_table, kv_lens=None, q_lens=None, causal: bool = True,
                        k_scale=None, v_scale=None) -> torch.Tensor:
    _no_grad_needed(q, k_pages, v_pages)
    torch._check(q.dim() == 4 and q.shape[-1] in (64, 128), lambda: "expected [B, Hq, Sq, 64|128]")
    torch._check(q.dtype in (torch.float16, torch.bfloat16), lambda: "expected fp16 or bf16")
    torch._check(block_table.dim() == 2, lambda: "expected a [B, max_pages_per_seq] block table")
    return torch.empty_like(q, memory_format=torch.contiguous_format)


_LIB.impl("prefill_paged", _prefill_paged_gpu, "CUDA")
_LIB.impl("prefill_paged", torch.library.fallthrough_kernel, "Autograd")
_LIB.impl("prefill_paged", _prefill_paged_cpu, "CPU")
torch.library.register_fake(PREFILL_PAGED_OP_NAME, _prefill_paged_fake, lib=_LIB)

prefill_paged = torch.ops.fa_mi355x.prefill_paged

# The packed (cu_seqlens) twins: q / k_new / v_new token-major [T,H,D], cu_seqlens
# int32 [B + 1] (required), B the caches' batch or the block table's rows:
# fa_mi355x.flash_attention_prefill_varlen[_paged] and
# flash_attention_cache_append_varlen[_paged] behind the same registrations as
# their padded twins.  Rows of the returned tensor that belong to no sequence
# are unspecified.
PREFILL_VARLEN_OP_NAME = "fa_mi355x::prefill_varlen"
_LIB.define("prefill_varlen(Tensor q, Tensor k_cache, Tensor v_cache, Tensor cu_seqlens_q, "
            "Tensor? kv_lens=None, bool causal=True, Tensor? k_scale=None, "
            "Tensor? v_scale=None) -> Tensor")


def _prefill_varlen_gpu(q, k_cache, v_cache, cu_seqlens_q, kv_lens=None, causal: bool = True,
                        k_scale=None, v_scale=None) -> torch.Tensor:
    _no_grad_needed(q, k_cache, v_cache)
    return flash_attention_prefill_varlen(q.contiguous(), k_cache, v_cache, cu_seqlens_q.contiguous(),
                                          None if kv_lens is None else kv_lens.contiguous(),
                                          causal=causal, k_scale=k_scale, v_scale=v_scale)


def _prefill_varlen_cpu(q, k_cache, v_cache, cu_seqlens_q, kv_lens=None, causal: bool = True,
                        k_scale=None, v_scale=None) -> torch.Tensor:
    raise ValueError("fa_mi355x::prefill_varlen needs GPU tensors (no CPU path)")


def _prefill_varlen_fake(q, k_cache, v_cache, cu_seqlens_q, kv_lens=None, causal: bool = True,
                         k_scale=None, v_scale=None) -> torch.Tensor:
    _no_grad_needed(q, k_cache, v_cache)
    torch._check(q.dim() == 3 and q.shape[-1] in (64, 128), lambda: "expected [T, Hq, 64|128]")
    torch._check(q.dtype in (torch.float16, torch.bfloat16), lambda: "expected fp16 or bf16")
    torch._check(cu_seqlens_q.dim() == 1, lambda: "expected a [B + 1] cu_seqlens_q")
    return torch.empty_like(q, memory_format=torch.contiguous_format)


_LIB.impl("prefill_varlen", _prefill_varlen_gpu, "CUDA")
_LIB.impl("prefill_varlen", torch.library.fallthrough_kernel, "Autograd")
_LIB.impl("prefill_varlen", _prefill_varlen_cpu, "CPU")
torch.library.register_fake(PREFILL_VARLEN_OP_NAME, _prefill_varlen_fake, lib=_LIB)

prefill_varlen = torch.ops.fa_mi355x.prefill_varlen

PREFILL_VARLEN_PAGED_OP_NAME = "fa_mi355x::prefill_varlen_paged"
_LIB.define("prefill_varlen_paged(Tensor q, Tensor k_pages, Tensor v_pages, Tensor block_table, "
            "Tensor cu_seqlens_q, Tensor? kv_lens=None, bool causal=True, Tensor? k_scale=None, "
            "Tensor? v_scale=None) -> Tensor")


def _prefill_varlen_paged_gpu(q, k_pages, v_pages, block_table, cu_seqlens_q, kv_lens=None,
                              causal: bool = True, k_scale=None, v_scale=None) -> torch.Tensor:
    _no_grad_needed(q, k_pages, v_pages)
    return flash_attention_prefill_varlen_paged(q.contiguous(), k_pages, v_pages,
                                                block_table.contiguous(), cu_seqlens_q.contiguous(),
                                                None if kv_lens is None else kv_lens.contiguous(),
                                                causal=causal, k_scale=k_scale, v_scale=v_scale)


def _prefill_varlen_paged_cpu(q, k_pages, v_pages, block_table, cu_seqlens_q, kv_lens=None,
                              causal: bool = True, k_scale=None, v_scale=None) -> torch.Tensor:
    raise ValueError("fa_mi355x::prefill_varlen_paged needs GPU tensors (no CPU path)")


def _prefill_varlen_paged_fake(q, k_pages, v_pages, block_table, cu_seqlens_q, kv_lens=None,
                               causal: bool = True, k_scale=None, v_scale=None) -> torch.Tensor:
    torch._check(block_table.dim() == 2, lambda: "expected a [B, max_pages_per_seq] block table")
    return _prefill_varlen_fake(q, k_pages, v_pages, cu_seqlens_q, kv_lens, causal, k_scale, v_scale)


_LIB.impl("prefill_varlen_paged", _prefill_varlen_paged_gpu, "CUDA")
_LIB.impl("prefill_varlen_paged", torch.library.fallthrough_kernel, "Autograd")
_LIB.impl("prefill_varlen_paged", _prefill_varlen_paged_cpu, "CPU")
torch.library.register_fake(PREFILL_VARLEN_PAGED_OP_NAME, _prefill_varlen_paged_fake, lib=_LIB)

prefill_varlen_paged = torch.ops.fa_mi355x.prefill_varlen_paged

CACHE_APPEND_VARLEN_OP_NAME = "fa_mi355x::cache_append_varlen"
_LIB.define("cache_append_varlen(Tensor k_new, Tensor v_new, Tensor(a!) k_cache, Tensor(b!) v_cache, "
            "Tensor cu_seqlens, Tensor kv_lens, Tensor? k_scale=None, Tensor? v_scale=None) -> ()")


def _cache_append_varlen_gpu(k_new, v_new, k_cache, v_cache, cu_seqlens, kv_lens, k_scale=None,
                             v_scale=None) -> None:
    flash_attention_cache_append_varlen(k_new.contiguous(), v_new.contiguous(), k_cache, v_cache,
                                        cu_seqlens.contiguous(), kv_lens.contiguous(),
                                        k_scale=k_scale, v_scale=v_scale)


def _cache_append_varlen_cpu(k_new, v_new, k_cache, v_cache, cu_seqlens, kv_lens, k_scale=None,
                             v_scale=None) -> None:
    raise ValueError("fa_mi355x::cache_append_varlen needs GPU tensors (no CPU path)")


def _cache_append_varlen_fake(k_new, v_new, k_cache, v_cache, cu_seqlens, kv_lens, k_scale=None,
                              v_scale=None) -> None:
    torch._check(k_new.dim() == 3 and k_new.shape[-1] in (64, 128), lambda: "expected [T, Hkv, 64|128]")
    torch._check(k_new.dtype in (torch.float16, torch.bfloat16), lambda: "expected fp16 or bf16")
    torch._check(k_cache.dim() == 4 and v_cache.dim() == 4, lambda: "expected 4-D caches")
    torch._check(cu_seqlens.dim() == 1, lambda: "expected a [B + 1] cu_seqlens")


_LIB.impl("cache_append_varlen", _cache_append_varlen_gpu, "CUDA")
_LIB.impl("cache_append_varlen", _cache_append_varlen_cpu, "CPU")
torch.library.register_fake(CACHE_APPEND_VARLEN_OP_NAME, _cache_append_varlen_fake, lib=_LIB)

cache_append_varlen = torch.ops.fa_mi355x.cache_append_varlen

CACHE_APPEND_VARLEN_PAGED_OP_NAME = "fa_mi355x::cache_append_varlen_paged"
_LIB.define("cache_append_varlen_paged(Tensor k_new, Tensor v_new, Tensor(a!) k_pages, "
            "Tensor(b!) v_pages, Tensor block_table, Tensor cu_seqlens, Tensor kv_lens, "
            "Tensor? k_scale=None, Tensor? v_scale=None) -> ()")


def _cache_append_varlen_paged_gpu(k_new, v_new, k_pages, v_pages, block_table, cu_seqlens, kv_lens,
                                   k_scale=None, v_scale=None) -> None:
    flash_attention_cache_append_varlen_paged(k_new.contiguous(), v_new.contiguous(), k_pages, v_pages,
                                              block_table.contiguous(), cu_seqlens.contiguous(),
                                              kv_lens.contiguous(), k_scale=k_scale, v_scale=v_scale)


def _cache_append_varlen_paged_cpu(k_new, v_new, k_pages, v_pages, block_table, cu_seqlens, kv_lens,
                                   k_scale=None, v_scale=None) -> None:
    raise ValueError("fa_mi355x::cache_append_varlen_paged needs GPU tensors (no CPU path)")


def _cache_append_varlen_paged_fake(k_new, v_new, k_pages, v_pages, block_table, cu_seqlens, kv_lens,
                                    k_scale=None, v_scale=None) -> None:
    _cache_append_varlen_fake(k_new, v_new, k_pages, v_pages, cu_seqlens, kv_lens, k_scale, v_scale)
    torch._check(block_table.dim() == 2, lambda: "expected a [B, max_pages_per_seq] block table")


_LIB.impl("cache_append_varlen_paged", _cache_append_varlen_paged_gpu, "CUDA")
_LIB.impl("cache_append_varlen_paged", _cache_append_varlen_paged_cpu, "CPU")
torch.library.register_fake(CACHE_APPEND_VARLEN_PAGED_OP_NAME, _cache_append_varlen_paged_fake, lib=_LIB)

cache_append_varlen_paged = torch.ops.fa_mi355x.cache_append_varlen_paged

# Sliding-window attention: the default overloads' schemas are pinned as they
# stand, so `window` comes in a `.window` overload of each of the six decode /
# prefill ops (the precedent is decode_paged.kv8): the default overload's
# arguments (decode_paged: the .kv8 overload's, with the scales), then
# `int window` (0: none; W >= 1: a row sees at most W keys, its own included,
# causal only).  A call through the packet that names or passes `window`
# resolves to it; every call an earlier overload accepts still resolves there.
_REQUIRED = object()


def _window_overload(name, args, wrapper, fake, overload="window"):
    """Registers fa_mi355x::<name>.window (or .<overload>).  args: the overload's arguments in
    order as (schema type, name, default) -- _REQUIRED for none -- which are
    also `wrapper`'s keyword names (the Python function the default overload
    calls); fake: the default overload's fake implementation.  Tensors are made
    contiguous but for the caches, which are taken as they are."""
    names = [n for _, n, _ in args]
    defaults = {n: d for _, n, d in args if d is not _REQUIRED}
    caches = set(names[1:3])

    def bind(a, kw):
        vals = dict(defaults)
        vals.update(zip(names, a))
        vals.update(kw)
        return vals

    def gpu(*a, **kw):
        vals = bind(a, kw)
        _no_grad_needed(*(vals[n] for n in names[:3]))
        for n, x in vals.items():
            if isinstance(x, torch.Tensor) and n not in caches and "scale" not in n:
                vals[n] = x.contiguous()
        return wrapper(**vals)

    def cpu(*a, **kw):
        raise ValueError("fa_mi355x::%s needs GPU tensors (no CPU path)" % name)

    def fake_impl(*a, **kw):
        vals = bind(a, kw)
        torch._check(vals.pop("window") >= 0, lambda: "expected window >= 0")
        sinks = vals.pop("sinks", None)
        torch._check(sinks is None or sinks.dim() == 1, lambda: "expected a [Hq] sinks")
        return fake(**vals)

    def lit(d):
        return "" if d is _REQUIRED else "=" + str(d)

    full = name + "." + overload
    _LIB.define("%s(%s) -> Tensor" % (full, ", ".join(f"{ty} {n}{lit(d)}" for ty, n, d in args)))
    _LIB.impl(full, gpu, "CUDA")
    _LIB.impl(full, torch.library.fallthrough_kernel, "Autograd")
    _LIB.impl(full, cpu, "CPU")
    torch.library.register_fake("fa_mi355x::" + full, fake_impl, lib=_LIB)


def _T(n):
    return ("Tensor", n, _REQUIRED)


def _opt(n):
    return ("Tensor?", n, None)


_TAIL = [("bool", "causal", True), _opt("k_scale"), _opt("v_scale"), ("int", "window", 0)]
_window_overload("decode", [_T("q"), _T("k_cache"), _T("v_cache"), _opt("kv_lens")] + _TAIL,
                 flash_attention_decode, _decode_fake)
_window_overload("decode_paged", [_T("q"), _T("k_pages"), _T("v_pages"), _T("block_table"), _opt("kv_lens")]
                 + _TAIL, flash_attention_decode_paged, _decode_paged_fake)
_window_overload("prefill", [_T("q"), _T("k_cache"), _T("v_cache"), _opt("kv_lens"), _opt("q_lens")] + _TAIL,
                 flash_attention_prefill, _prefill_fake)
_window_overload("prefill_paged", [_T("q"), _T("k_pages"), _T("v_pages"), _T("block_table"), _opt("kv_lens"),
                                   _opt("q_lens")] + _TAIL, flash_attention_prefill_paged, _prefill_paged_fake)
_window_overload("prefill_varlen", [_T("q"), _T("k_cache"), _T("v_cache"), _T("cu_seqlens_q"), _opt("kv_lens")]
                 + _TAIL, flash_attention_prefill_varlen, _prefill_varlen_fake)
_window_overload("prefill_varlen_paged", [_T("q"), _T("k_pages"), _T("v_pages"), _T("block_table"),
                                          _T("cu_seqlens_q"), _opt("kv_lens")] + _TAIL,
                 flash_attention_prefill_varlen_paged, _prefill_varlen_paged_fake)

# Attention sinks: a `.sinks` overload of the same six ops, the `.window`
# overload's arguments and then `Tensor? sinks=None` (float32 [Hq]: one logit
# per query head that joins the softmax denominator and contributes no value;
# the Python functions' `sinks`).  Registered after `.window`, so a call
# that names or passes `sinks` resolves to it and every call an earlier overload
# accepts still resolves there.
_SINKS = _TAIL + [_opt("sinks")]
_window_overload("decode", [_T("q"), _T("k_cache"), _T("v_cache"), _opt("kv_lens")] + _SINKS,
                 flash_attention_decode, _decode_fake, "sinks")
_window_overload("decode_paged", [_T("q"), _T("k_pages"), _T("v_pages"), _T("block_table"), _opt("kv_lens")]
                 + _SINKS, flash_attention_decode_paged, _decode_paged_fake, "sinks")
_window_overload("prefill", [_T("q"), _T("k_cache"), _T("v_cache"), _opt("kv_lens"), _opt("q_lens")] + _SINKS,
                 flash_attention_prefill, _prefill_fake, "sinks")
_window_overload("prefill_paged", [_T("q"), _T("k_pages"), _T("v_pages"), _T("block_table"), _opt("kv_lens"),
                                   _opt("q_lens")] + _SINKS, flash_attention_prefill_paged, _prefill_paged_fake,
                 "sinks")
_window_overload("prefill_varlen", [_T("q"), _T("k_cache"), _T("v_cache"), _T("cu_seqlens_q"), _opt("kv_lens")]
                 + _SINKS, flash_attention_prefill_varlen, _prefill_varlen_fake, "sinks")
_window_overload("prefill_varlen_paged", [_T("q"), _T("k_pages"), _T("v_pages"), _T("block_table"),
                                          _T("cu_seqlens_q"), _opt("kv_lens")] + _SINKS,
                 flash_attention_prefill_varlen_paged, _prefill_varlen_paged_fake, "sinks")

# Fused RoPE + cache append: rope_append(q, k_new, v_new, the caches, kv_lens,
# cos, sin: float32 [rope_len, R/2]) and its paged / packed twins:
# fa_mi355x.flash_attention_rope_append[_varlen][_paged] behind the
# cache_append kind of registration.  The caches are mutated in place and the
# rotated Q comes back as a NEW tensor (the functions' q_out=None; for the
# in-place form call the Python function with q_out=q).
_ROPE_TAIL = ("Tensor cos, Tensor sin, {lens}bool interleaved=False, Tensor? k_scale=None, "
              "Tensor? v_scale=None) -> Tensor")


def _rope_op(name, fn, cache_args, packed):
    """Registers fa_mi355x::<name>.  cache_args: the schema's names between
    v_new and cos, in the Python function's order; `packed`: q / k_new / v_new
    are [T,H,D] and there is no new_lens."""
    names = cache_args.replace("Tensor(a!) ", "").replace("Tensor(b!) ", "").replace("Tensor ", "").split(", ")
    _LIB.define(f"{name}(Tensor q, Tensor k_new, Tensor v_new, {cache_args}, "
                + _ROPE_TAIL.format(lens="" if packed else "Tensor? new_lens=None, "))
    rank = 3 if packed else 4
    # the op's arguments in order: they are the Python function's keyword names
    order = (["q", "k_new", "v_new"] + names + ["cos", "sin"] + ([] if packed else ["new_lens"])
             + ["interleaved", "k_scale", "v_scale"])

    def bind(args, kw):
        a = dict(zip(order, args))
        a.update(kw)
        return a

    def gpu(*args, **kw):
        a = bind(args, kw)
        # the caches are taken as they are (a strided cache raises), the rest made contiguous
        a = {k: (v.contiguous() if isinstance(v, torch.Tensor) and k not in names[:2] else v)
             for k, v in a.items()}
        return fn(**a)

    def cpu(*args, **kw):
        raise ValueError(f"fa_mi355x::{name} needs GPU tensors (no CPU path)")

    def fake(*args, **kw):
        a = bind(args, kw)
        q, k_new = a["q"], a["k_new"]
        torch._check(k_new.dim() == rank and k_new.shape[-1] in (64, 128),
                     lambda: "expected [T, Hkv, 64|128]" if packed else "expected [B, Hkv, Sn, 64|128]")
        torch._check(k_new.dtype in (torch.float16, torch.bfloat16), lambda: "expected fp16 or bf16")
        torch._check(q.dim() == rank and q.dtype == k_new.dtype, lambda: "expected q like k_new but for the heads")
        torch._check(a[names[0]].dim() == 4 and a[names[1]].dim() == 4, lambda: "expected 4-D caches")
        if "block_table" in a:
            torch._check(a["block_table"].dim() == 2, lambda: "expected a [B, max_pages_per_seq] block table")
        torch._check(a["cos"].dim() == 2 and a["cos"].dtype == torch.float32,
                     lambda: "expected float32 [rope_len, R/2] tables")
        return torch.empty_like(q, memory_format=torch.contiguous_format)

    _LIB.impl(name, gpu, "CUDA")
    _LIB.impl(name, cpu, "CPU")
    torch.library.register_fake("fa_mi355x::" + name, fake, lib=_LIB)


_rope_op("rope_append", flash_attention_rope_append,
         "Tensor(a!) k_cache, Tensor(b!) v_cache, Tensor kv_lens", False)
_rope_op("rope_append_paged", flash_attention_rope_append_paged,
         "Tensor(a!) k_pages, Tensor(b!) v_pages, Tensor block_table, Tensor kv_lens", False)
_rope_op("rope_append_varlen", flash_attention_rope_append_varlen,
         "Tensor(a!) k_cache, Tensor(b!) v_cache, Tensor cu_seqlens, Tensor kv_lens", True)
_rope_op("rope_append_varlen_paged", flash_attention_rope_append_varlen_paged,
         "Tensor(a!) k_pages, Tensor(b!) v_pages, Tensor block_table, Tensor cu_seqlens, Tensor kv_lens", True)

rope_append = torch.ops.fa_mi355x.rope_append
rope_append_paged = torch.ops.fa_mi355x.rope_append_paged
rope_append_varlen = torch.ops.fa_mi355x.rope_append_varlen
rope_append_varlen_paged = torch.ops.fa_mi355x.rope_append_varlen_paged

# Attention over token-major Q, K and V with no cache: attn_varlen(q [T_q,Hq,D],
# k / v [T_k,Hkv,D], cu_seqlens_q int32 [B + 1], cu_seqlens_k or None = self-
# attention) and attn_bshd(q [B,Sq,Hq,D], k / v [B,Sk,Hkv,D]):
# fa_mi355x.flash_attention_varlen / flash_attention_bshd behind the prefill
# kind of registration, each with a `.window` overload (then `int window`) and
# a `.sinks` overload (then `Tensor? sinks`), registered in that order so that
# every call an earlier overload accepts still resolves there.  q, k and v are
# taken as they are -- a token-major view (the slices of a fused QKV buffer) is
# read in place and any other layout raises, nothing is copied; rows of the
# returned tensor that belong to no sequence are unspecified.


def _attn_op(name, fn, head, rank):
    """Registers fa_mi355x::<name> and its .window / .sinks overloads.  head: the
    schema's arguments before `causal`, which are `fn`'s first positionals."""
    names = [a.split()[-1].split("=")[0] for a in head]
    layout = "[T, H, 64|128]" if rank == 3 else "[B, S, H, 64|128]"

    def fake(*args, **kw):
        vals = dict(zip(names + ["causal", "window", "sinks"], args))
        vals.update(kw)
        q, k, v = vals["q"], vals["k"], vals["v"]
        _no_grad_needed(q, k, v)
        torch._check(q.dim() == rank and q.shape[-1] in (64, 128), lambda: "expected q " + layout)
        torch._check(k.dim() == rank and v.dim() == rank, lambda: "expected k, v " + layout)
        torch._check(q.dtype in (torch.float16, torch.bfloat16), lambda: "expected fp16 or bf16")
        if rank == 3:
            torch._check(vals["cu_seqlens_q"].dim() == 1, lambda: "expected a [B + 1] cu_seqlens_q")
        torch._check(vals.get("window", 0) >= 0, lambda: "expected window >= 0")
        sinks = vals.get("sinks")
        torch._check(sinks is None or sinks.dim() == 1, lambda: "expected a [Hq] sinks")
        return torch.empty(q.shape, dtype=q.dtype, device=q.device)

    def gpu(*args, **kw):
        vals = dict(zip(names + ["causal", "window", "sinks"], args))
        vals.update(kw)
        _no_grad_needed(vals["q"], vals["k"], vals["v"])
        for n in ("cu_seqlens_q", "cu_seqlens_k", "sinks"):
            if isinstance(vals.get(n), torch.Tensor):
                vals[n] = vals[n].contiguous()
        return fn(**vals)

    def cpu(*args, **kw):
        raise ValueError("fa_mi355x::%s needs GPU tensors (no CPU path)" % name)

    for overload, tail in (("", []), (".window", ["int window=0"]),
                           (".sinks", ["int window=0", "Tensor? sinks=None"])):
        full = name + overload
        _LIB.define("%s(%s) -> Tensor" % (full, ", ".join(head + ["bool causal=False"] + tail)))
        _LIB.impl(full, gpu, "CUDA")
        _LIB.impl(full, torch.library.fallthrough_kernel, "Autograd")
        _LIB.impl(full, cpu, "CPU")
        torch.library.register_fake("fa_mi355x::" + full, fake, lib=_LIB)


_attn_op("attn_varlen", flash_attention_varlen,
         ["Tensor q", "Tensor k", "Tensor v", "Tensor cu_seqlens_q", "Tensor? cu_seqlens_k=None"], 3)
_attn_op("attn_bshd", flash_attention_bshd, ["Tensor q", "Tensor k", "Tensor v"], 4)

attn_varlen = torch.ops.fa_mi355x.attn_varlen
attn_bshd = torch.ops.fa_mi355x.attn_bshd

# The backward pass of those two and the differentiable functions over it.
# attn_varlen_fwd / attn_bshd_fwd return (out, lse) -- the forward with
# return_lse=True as an op, so that it has a fake implementation; attn_varlen_bwd
# / attn_bshd_bwd(dout, q, k, v, out, lse, ...) return (dq, dk, dv):
# fa_mi355x.flash_attention_varlen_backward / flash_attention_bshd_backward.
# Everything is taken as it is (views under the stride rule, nothing copied).
# Each of the four has a `.window` overload (then `int window=0`) and a `.sinks`
# overload (then `Tensor? sinks=None`), registered after the base schema as for
# attn_varlen above; the `.sinks` backward returns (dq, dk, dv, dsinks), dsinks
# float32 [Hq] (zeros when sinks is None).
# attn_varlen / attn_bshd above stay forward-only and keep raising on inputs
# that require grad; the differentiable entry points are flash_attn_varlen_func
# and flash_attn_func below.


def _attn_grad_ops(name, fwd_fn, bwd_fn, mid, rank):
    """Registers fa_mi355x::<name>_fwd and <name>_bwd.  mid: the schema's
    arguments between v (forward) / lse (backward) and `causal`."""
    mid_names = [a.split()[-1].split("=")[0] for a in mid]
    layout = "[T, H, 64|128]" if rank == 3 else "[B, S, H, 64|128]"
    fwd_names = ["q", "k", "v"] + mid_names + ["causal", "window", "sinks"]
    bwd_names = ["dout", "q", "k", "v", "out", "lse"] + mid_names + ["causal", "window", "sinks"]

    def check(q, k, v, vals):
        torch._check(q.dim() == rank and q.shape[-1] in (64, 128), lambda: "expected q " + layout)
        torch._check(k.dim() == rank and v.dim() == rank and k.shape == v.shape,
                     lambda: "expected k, v " + layout)
        torch._check(q.dtype in (torch.float16, torch.bfloat16), lambda: "expected fp16 or bf16")
        if rank == 3:
            torch._check(vals["cu_seqlens_q"].dim() == 1, lambda: "expected a [B + 1] cu_seqlens_q")
        torch._check(vals.get("window", 0) >= 0, lambda: "expected window >= 0")
        sinks = vals.get("sinks")
        torch._check(sinks is None or (sinks.dim() == 1 and sinks.dtype == torch.float32),
                     lambda: "expected a float32 [Hq] sinks")

    def bind(names, args, kw):
        vals = dict(zip(names, args))
        vals.update(kw)
        for n in mid_names + ["sinks"]:
            if isinstance(vals.get(n), torch.Tensor):
                vals[n] = vals[n].contiguous()
        return vals

    def new_lse(q):
        if rank == 3:
            return torch.empty((q.shape[1], q.shape[0]), dtype=torch.float32, device=q.device)
        b, sq, hq = q.shape[0], q.shape[1], q.shape[2]
        return torch.empty((hq, b * sq), dtype=torch.float32, device=q.device).view(hq, b, sq).permute(1, 0, 2)

    def fwd_gpu(*args, **kw):
        out, lse = fwd_fn(**bind(fwd_names, args, kw), return_lse=True)
        return out, lse

    def fwd_fake(*args, **kw):
        vals = bind(fwd_names, args, kw)
        q = vals["q"]
        check(q, vals["k"], vals["v"], vals)
        return torch.empty(q.shape, dtype=q.dtype, device=q.device), new_lse(q)

    def bwd_gpu(*args, **kw):
        return bwd_fn(**bind(bwd_names, args, kw))

    def new_dsinks(q):
        return torch.empty((q.shape[-2],), dtype=torch.float32, device=q.device)

    def bwd_sinks_gpu(*args, **kw):
        vals = bind(bwd_names, args, kw)
        g = bwd_fn(**vals)
        # four tensors whatever `sinks` is: without sinks their gradient is zeros
        return g if len(g) == 4 else (*g, new_dsinks(vals["q"]).zero_())

    def bwd_sinks_fake(*args, **kw):
        return (*bwd_fake(*args, **kw), new_dsinks(bind(bwd_names, args, kw)["q"]))

    def bwd_fake(*args, **kw):
        vals = bind(bwd_names, args, kw)
        q, k, v = vals["q"], vals["k"], vals["v"]
        check(q, k, v, vals)
        torch._check(vals["dout"].shape == q.shape and vals["out"].shape == q.shape,
                     lambda: "expected dout and out shaped like q")
        torch._check(vals["lse"].dtype == torch.float32 and vals["lse"].shape == new_lse(q).shape,
                     lambda: "expected the forward's float32 lse")
        return tuple(torch.empty(t.shape, dtype=q.dtype, device=q.device) for t in (q, k, v))

    def cpu_of(full):
        def cpu(*args, **kw):
            raise ValueError("fa_mi355x::%s needs GPU tensors (no CPU path)" % full)
        return cpu

    for overload, more in (("", []), (".window", ["int window=0"]),
                           (".sinks", ["int window=0", "Tensor? sinks=None"])):
        tail = ", ".join(mid + ["bool causal=False"] + more)
        four = overload == ".sinks"
        for full, schema, gpu, fake in (
                (name + "_fwd", "Tensor q, Tensor k, Tensor v, %s) -> (Tensor, Tensor)" % tail, fwd_gpu, fwd_fake),
                (name + "_bwd", "Tensor dout, Tensor q, Tensor k, Tensor v, Tensor out, Tensor lse, %s) -> "
                                "(Tensor, Tensor, Tensor%s)" % (tail, ", Tensor" if four else ""),
                 bwd_sinks_gpu if four else bwd_gpu, bwd_sinks_fake if four else bwd_fake)):
            _LIB.define(full + overload + "(" + schema)
            _LIB.impl(full + overload, gpu, "CUDA")
            _LIB.impl(full + overload, cpu_of(full), "CPU")
            torch.library.register_fake("fa_mi355x::" + full + overload, fake, lib=_LIB)


_attn_grad_ops("attn_varlen", flash_attention_varlen, flash_attention_varlen_backward,
               ["Tensor cu_seqlens_q", "Tensor? cu_seqlens_k=None"], 3)
_attn_grad_ops("attn_bshd", flash_attention_bshd, flash_attention_bshd_backward, [], 4)

attn_varlen_fwd = torch.ops.fa_mi355x.attn_varlen_fwd
attn_varlen_bwd = torch.ops.fa_mi355x.attn_varlen_bwd
attn_bshd_fwd = torch.ops.fa_mi355x.attn_bshd_fwd
attn_bshd_bwd = torch.ops.fa_mi355x.attn_bshd_bwd


def _dout_as_given_or_dense(dout, rank):
    """dout under the stride rule as it is; otherwise contiguous -- the one
    documented copy of the backward, made here and nowhere below."""
    try:
        _token_stride(dout, "dout", rank)
    except FlashAttentionError:
        return dout.contiguous()
    return dout


class _FlashAttnVarlen(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, cu_seqlens_q, cu_seqlens_k, causal):
        out, lse = attn_varlen_fwd(q, k, v, cu_seqlens_q, cu_seqlens_k, causal)
        ctx.save_for_backward(q, k, v, out, lse, cu_seqlens_q, cu_seqlens_k)
        ctx.causal = causal
        return out

    @staticmethod
    def backward(ctx, dout):
        q, k, v, out, lse, cu_q, cu_k = ctx.saved_tensors
        dq, dk, dv = attn_varlen_bwd(_dout_as_given_or_dense(dout, 3), q, k, v, out, lse, cu_q, cu_k,
                                     ctx.causal)
        return dq, dk, dv, None, None, None


class _FlashAttn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, causal):
        out, lse = attn_bshd_fwd(q, k, v, causal)
        ctx.save_for_backward(q, k, v, out, lse)
        ctx.causal = causal
        return out

    @staticmethod
    def backward(ctx, dout):
        q, k, v, out, lse = ctx.saved_tensors
        dq, dk, dv = attn_bshd_bwd(_dout_as_given_or_dense(dout, 4), q, k, v, out, lse, ctx.causal)
        return dq, dk, dv, None


# With a window or sinks: the same two Functions over the `.window` / `.sinks`
# overloads.  `sinks` is a differentiable input; its gradient is the backward's dsinks.


def _masked_forward(ctx, op, args, causal, window, sinks):
    """The `.window` / `.sinks` overload of a forward op; saves what its backward reads."""
    last = () if sinks is None else (sinks,)
    out, lse = (op.window if sinks is None else op.sinks)(*args, causal, window, *last)
    ctx.save_for_backward(*args[:3], out, lse, *args[3:], *last)
    ctx.causal, ctx.window, ctx.has_sinks = causal, window, sinks is not None
    return out


def _masked_backward(ctx, op, dout, rank):
    """(dq, dk, dv, dsinks or None) of the `.window` / `.sinks` overload of a backward op."""
    saved = ctx.saved_tensors
    last = (saved[-1],) if ctx.has_sinks else ()
    rest = saved[:len(saved) - len(last)]
    g = (op.sinks if ctx.has_sinks else op.window)(_dout_as_given_or_dense(dout, rank), *rest, ctx.causal,
                                                   ctx.window, *last)
    return g if ctx.has_sinks else (*g, None)


class _FlashAttnVarlenMasked(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, cu_seqlens_q, cu_seqlens_k, causal, window, sinks):
        return _masked_forward(ctx, attn_varlen_fwd, (q, k, v, cu_seqlens_q, cu_seqlens_k), causal, window, sinks)

    @staticmethod
    def backward(ctx, dout):
        dq, dk, dv, dsinks = _masked_backward(ctx, attn_varlen_bwd, dout, 3)
        return dq, dk, dv, None, None, None, None, dsinks


class _FlashAttnMasked(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, causal, window, sinks):
        return _masked_forward(ctx, attn_bshd_fwd, (q, k, v), causal, window, sinks)

    @staticmethod
    def backward(ctx, dout):
        dq, dk, dv, dsinks = _masked_backward(ctx, attn_bshd_bwd, dout, 4)
        return dq, dk, dv, None, None, dsinks


def flash_attn_varlen_func(q, k, v, cu_seqlens_q, cu_seqlens_k=None, causal: bool = False, window: int = 0,
                           sinks=None):
    """Differentiable fa_mi355x.flash_attention_varlen (see fa_mi355x.flash_attn_varlen_func)."""
    if window == 0 and sinks is None:
        return _FlashAttnVarlen.apply(q, k, v, cu_seqlens_q, cu_seqlens_k, bool(causal))
    return _FlashAttnVarlenMasked.apply(q, k, v, cu_seqlens_q, cu_seqlens_k, bool(causal), window, sinks)


def flash_attn_func(q, k, v, causal: bool = False, window: int = 0, sinks=None):
    """Differentiable fa_mi355x.flash_attention_bshd (see fa_mi355x.flash_attn_func)."""
    if window == 0 and sinks is None:
        return _FlashAttn.apply(q, k, v, bool(causal))
    return _FlashAttnMasked.apply(q, k, v, bool(causal), window, sinks)
