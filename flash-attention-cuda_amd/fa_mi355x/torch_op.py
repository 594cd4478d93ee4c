"""PyTorch custom operators over the MI355X kernels (SURVEY.md §8(f) rank 3:
the wrapper that puts the kernels beside PyTorch SDPA on one box).

    import fa_mi355x.torch_op  # registers torch.ops.fa_mi355x.*
    o = torch.ops.fa_mi355x.fwd(q, k, v, causal=True)  # [B,H,S,D]
    o = torch.ops.fa_mi355x.decode(q, k_cache, v_cache, kv_lens, causal=True)
    o = torch.ops.fa_mi355x.decode_paged(q, k_pages, v_pages, block_table, kv_lens, causal=True)
    o = torch.ops.fa_mi355x.decode(q, k8_cache, v8_cache, kv_lens, k_scale=ks, v_scale=vs)  # FP8 cache
    o = torch.ops.fa_mi355x.prefill(q, k_cache, v_cache, kv_lens, q_lens, causal=True)  # any Sq
    o = torch.ops.fa_mi355x.prefill_varlen(q_packed, k_cache, v_cache, cu_seqlens_q, kv_lens)  # [T,Hq,D]
    torch.ops.fa_mi355x.cache_append(k_new, v_new, k_cache, v_cache, kv_lens)  # writes the caches
    q_rot = torch.ops.fa_mi355x.rope_append(q, k_new, v_new, k_cache, v_cache, kv_lens, cos, sin)  # RoPE + append
    o = torch.ops.fa_mi355x.attn_varlen(q, k, v, cu_seqlens_q, cu_seqlens_k, causal=False)  # [T,H,D], no cache
    o = torch.ops.fa_mi355x.attn_bshd(q, k, v, causal=True)  # [B,S,H,D], no cache
    out, lse = torch.ops.fa_mi355x.attn_varlen_fwd(q, k, v, cu_seqlens_q, cu_seqlens_k)
    dq, dk, dv = torch.ops.fa_mi355x.attn_varlen_bwd(dout, q, k, v, out, lse, cu_seqlens_q, cu_seqlens_k)
    o = fa_mi355x.flash_attn_varlen_func(q, k, v, cu_seqlens_q, causal=True, window=128, sinks=sinks)

Every op is a row of the table ``_OPS`` below: its arguments, composed from
named groups, and the fa_mi355x function it wraps, whose keyword names the
arguments are and whose docstring says what they mean.  Each op with a cache
has a ``_paged`` twin (the pools and the block table in the caches' place),
prefill, cache_append and rope_append a ``_varlen`` twin (token-major [T,H,D]
and cu_seqlens).  The rules, once:

* Registration.  The schema is defined with ``torch.library.Library`` and the
  kernel registered for the CUDA dispatch key directly (``custom_op``'s extra
  dispatch layers cost 3.7 us more per call, 12.2 vs 8.5 us host time on a
  short launch, tools/host_overhead.py).  A fake implementation supplies the
  output's shape, so an op is opaque to ``torch.compile``; it launches on the
  current HIP stream, so it can be captured in a HIP graph.  It calls the same
  C ABI as every other entry point.  There is no CPU or eager fallback: a CPU
  tensor raises ValueError.
* Forward only.  fwd, decode*, prefill*, attn_varlen and attn_bshd have no
  backward: their Autograd key falls through (no Python frame on the call
  path) and their GPU and fake kernels raise when a gradient would be needed
  (one of the first three arguments requiring grad with grad mode on), where
  an output that backward silently ignores would come back otherwise.  The
  appends mutate their caches in place and return nothing (rope_append: the
  rotated Q as a new tensor).  The differentiable attention is
  flash_attn_varlen_func / flash_attn_func at the end of this module,
  torch.autograd.Functions over the attn_*_fwd / attn_*_bwd ops.
* As-is arguments.  Each row names the arguments passed on as they are; every
  other tensor is made contiguous.  Caches and pools are always as they are:
  a strided view (a slice of a larger cache) raises FlashAttentionError where
  a copy would move the whole cache once more than the kernel does.  So are q,
  k, v, dout, out and lse of the attention with no cache: a token-major view
  (the slices of a fused QKV buffer) is read in place, any other layout raises.
* Overload order.  A default overload's schema is pinned as it stands, so a
  later argument comes in a further overload: the default's arguments plus a
  group.  ``.kv8`` (decode_paged only) adds the FP8 pools' scales, ``.window``
  adds ``int window`` (0: none; W >= 1: a row sees at most W keys, its own
  included, causal only), ``.sinks`` adds ``Tensor? sinks`` after it (float32
  [Hq]: one logit per query head that joins the softmax denominator and
  contributes no value).  They are registered in that order and a call through
  the packet resolves to the first overload that accepts it, so every call an
  earlier overload accepts still resolves there.  The ``.sinks`` overload of a
  backward returns (dq, dk, dv, dsinks), dsinks float32 [Hq], zeros when sinks
  is None.
"""
from __future__ import annotations

import inspect
from dataclasses import dataclass
from functools import partial, wraps
from typing import Callable

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
DECODE_OP_NAME = "fa_mi355x::decode"
DECODE_PAGED_OP_NAME = "fa_mi355x::decode_paged"

_LIB = torch.library.Library("fa_mi355x", "DEF")

# An argument is (schema type, name, default), _REQUIRED for no default; the
# name is also the wrapped function's keyword.
_REQUIRED = object()


def _T(name, mutated=""):
    """A required tensor; mutated: the "(a!)" / "(b!)" of a cache written in place."""
    return ("Tensor" + mutated, name, _REQUIRED)


def _opt(name):
    return ("Tensor?", name, None)


# The groups the argument lists are composed from (csrc/fa_decode_host.hpp has the C side's).
_QKV = [_T("q"), _T("k"), _T("v")]
_NEW = [_T("k_new"), _T("v_new")]
_CACHE = [_T("k_cache"), _T("v_cache")]
_PAGES = [_T("k_pages"), _T("v_pages"), _T("block_table")]
_CACHE_OUT = [_T("k_cache", "(a!)"), _T("v_cache", "(b!)")]
_PAGES_OUT = [_T("k_pages", "(a!)"), _T("v_pages", "(b!)"), _T("block_table")]
_KV_LENS, _Q_LENS, _NEW_LENS = _opt("kv_lens"), _opt("q_lens"), _opt("new_lens")
_CU_Q, _CU_K, _CU = _T("cu_seqlens_q"), _opt("cu_seqlens_k"), _T("cu_seqlens")
_CAUSAL, _NOT_CAUSAL = ("bool", "causal", True), ("bool", "causal", False)
_SCALES = [_opt("k_scale"), _opt("v_scale")]
_WINDOW = [("int", "window", 0)]
_SINKS = _WINDOW + [_opt("sinks")]
_ROPE = [_T("cos"), _T("sin")]
_ROPE_TAIL = [("bool", "interleaved", False)] + _SCALES

# The arguments passed on as they are.  The rope ops make the scales contiguous
# where the other cache ops pass them on: inherited, kept as it was.
_CACHES_AS_IS = {"k_cache", "v_cache", "k_pages", "v_pages"}
_CACHE_OPS_AS_IS = _CACHES_AS_IS | {"k_scale", "v_scale"}
_ATTN_AS_IS = {"q", "k", "v", "dout", "out", "lse"}


@dataclass
class _Op:
    """One overload.  fn: the Python function it calls, whose parameters of the
    arguments' names have the arguments' defaults; fake: its fake check, called
    with {name: value} and returning the fake output."""
    packet: str
    overload: str  # "" for the default
    args: list
    fn: Callable
    fake: Callable
    as_is: set = frozenset(_CACHE_OPS_AS_IS)
    returns: str = "Tensor"
    forward_only: bool = True  # the Autograd fallthrough and the forward-only guard


def _no_grad_needed(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor) -> None:
    if torch.is_grad_enabled() and (q.requires_grad or k.requires_grad or v.requires_grad):
        raise RuntimeError("fa_mi355x::fwd is forward-only (no backward): call it under "
                           "torch.no_grad() / inference_mode or on tensors that do not require grad")


def _register(op: _Op, lib=None, ns: str = "fa_mi355x") -> None:
    """Defines fa_mi355x::<packet>[.<overload>] and registers its CUDA, CPU, fake
    and (forward_only) Autograd kernels.  lib, ns: another module's library and
    its namespace (torch_op_tree.py), under the same rules."""
    lib = _LIB if lib is None else lib
    full = op.packet + ("." + op.overload if op.overload else "")
    names = [n for _, n, _ in op.args]
    defaults = {n: d for _, n, d in op.args if d is not _REQUIRED}
    fn, fake, guarded = op.fn, op.fake, op.forward_only
    # The dispatcher hands a kernel positionals only and leaves out the trailing
    # ones that equal their defaults, which are fn's own defaults too.  So the call
    # path is a few list operations: the given arguments go to fn as they come,
    # positionally as far as fn's parameters are the schema's (`lead` of them) and
    # by keyword after that; dense[n] holds the positions to make contiguous
    # among n given arguments.
    params = inspect.signature(fn).parameters
    if any(params[n].default != d for n, d in defaults.items()):
        raise TypeError("fa_mi355x::%s: a default differs from %s's" % (full, fn))
    lead = 0
    for p, n in zip(params.values(), names):
        if p.name != n or p.kind is not p.POSITIONAL_OR_KEYWORD:
            break
        lead += 1
    keywords = names[lead:]
    dense = [[i for i, (ty, n, _) in enumerate(op.args[:given]) if ty.startswith("Tensor") and n not in op.as_is]
             for given in range(len(names) + 1)]

    def gpu(*a):
        if guarded:
            _no_grad_needed(a[0], a[1], a[2])
        vals = list(a)
        for i in dense[len(a)]:
            x = a[i]
            if x is not None:
                vals[i] = x.contiguous()
        if len(a) <= lead:
            return fn(*vals)
        return fn(*vals[:lead], **dict(zip(keywords, vals[lead:])))

    def cpu(*a, **kw):
        raise ValueError("%s::%s needs GPU tensors (no CPU path)" % (ns, op.packet))

    def fake_impl(*a, **kw):
        vals = {**defaults, **dict(zip(names, a)), **kw}
        if guarded:
            _no_grad_needed(*(vals[n] for n in names[:3]))
        return fake(vals)

    schema = ", ".join("%s %s%s" % (ty, n, "" if d is _REQUIRED else "=" + str(d)) for ty, n, d in op.args)
    lib.define("%s(%s) -> %s" % (full, schema, op.returns))
    lib.impl(full, gpu, "CUDA")
    if guarded:
        lib.impl(full, torch.library.fallthrough_kernel, "Autograd")
    lib.impl(full, cpu, "CPU")
    torch.library.register_fake(ns + "::" + full, fake_impl, lib=lib)


# The fake checks, one per family.


def _check_half(x, rank, layout):
    torch._check(x.dim() == rank and x.shape[-1] in (64, 128), lambda: "expected " + layout)
    torch._check(x.dtype in (torch.float16, torch.bfloat16), lambda: "expected fp16 or bf16")


def _check_caches(a):
    k, v = (a["k_pages"], a["v_pages"]) if "k_pages" in a else (a["k_cache"], a["v_cache"])
    torch._check(k.dim() == 4 and v.dim() == 4, lambda: "expected 4-D caches")


def _check_block_table(a):
    if "block_table" in a:
        torch._check(a["block_table"].dim() == 2, lambda: "expected a [B, max_pages_per_seq] block table")


def _fwd_fake(a):
    _check_half(a["q"], 4, "[B, H, S, 64|128]")
    return torch.empty_like(a["q"], memory_format=torch.contiguous_format)


def _cache_read_fake(a):
    """decode* and prefill*: q is packed [T,Hq,D] where there is a cu_seqlens_q."""
    torch._check(a.get("window", 0) >= 0, lambda: "expected window >= 0")
    sinks = a.get("sinks")
    torch._check(sinks is None or sinks.dim() == 1, lambda: "expected a [Hq] sinks")
    if "cu_seqlens_q" in a:
        _check_half(a["q"], 3, "[T, Hq, 64|128]")
        torch._check(a["cu_seqlens_q"].dim() == 1, lambda: "expected a [B + 1] cu_seqlens_q")
    else:
        _check_half(a["q"], 4, "[B, Hq, Sq, 64|128]")
    _check_block_table(a)
    return torch.empty_like(a["q"], memory_format=torch.contiguous_format)


def _check_new(a):
    """k_new of cache_append* and rope_append*: packed [T,Hkv,D] where there is a cu_seqlens."""
    if "cu_seqlens" in a:
        _check_half(a["k_new"], 3, "[T, Hkv, 64|128]")
    else:
        _check_half(a["k_new"], 4, "[B, Hkv, Sn, 64|128]")


def _append_fake(a):
    _check_new(a)
    _check_caches(a)
    if "cu_seqlens" in a:
        torch._check(a["cu_seqlens"].dim() == 1, lambda: "expected a [B + 1] cu_seqlens")
    _check_block_table(a)


def _rope_fake(a):
    _check_new(a)
    q = a["q"]
    torch._check(q.dim() == a["k_new"].dim() and q.dtype == a["k_new"].dtype,
                 lambda: "expected q like k_new but for the heads")
    _check_caches(a)
    _check_block_table(a)
    torch._check(a["cos"].dim() == 2 and a["cos"].dtype == torch.float32,
                 lambda: "expected float32 [rope_len, R/2] tables")
    return torch.empty_like(q, memory_format=torch.contiguous_format)


def _check_attn(a, grad):
    """q, k, v, cu_seqlens_q, window and sinks of the attention with no cache
    (rank 3 where there is a cu_seqlens_q); grad: of the _fwd / _bwd ops."""
    q, k, v = a["q"], a["k"], a["v"]
    rank, layout = (3, "[T, H, 64|128]") if "cu_seqlens_q" in a else (4, "[B, S, H, 64|128]")
    torch._check(q.dim() == rank and q.shape[-1] in (64, 128), lambda: "expected q " + layout)
    torch._check(k.dim() == rank and v.dim() == rank and (not grad or k.shape == v.shape),
                 lambda: "expected k, v " + layout)
    torch._check(q.dtype in (torch.float16, torch.bfloat16), lambda: "expected fp16 or bf16")
    if rank == 3:
        torch._check(a["cu_seqlens_q"].dim() == 1, lambda: "expected a [B + 1] cu_seqlens_q")
    torch._check(a.get("window", 0) >= 0, lambda: "expected window >= 0")
    sinks = a.get("sinks")
    if grad:
        torch._check(sinks is None or (sinks.dim() == 1 and sinks.dtype == torch.float32),
                     lambda: "expected a float32 [Hq] sinks")
    else:
        torch._check(sinks is None or sinks.dim() == 1, lambda: "expected a [Hq] sinks")
    return q


def _new_lse(q):
    """The forward's LSE: [Hq, T], or of q [B,Sq,Hq,D] the [B, Hq, Sq] view of [Hq, B*Sq]."""
    if q.dim() == 3:
        return torch.empty((q.shape[1], q.shape[0]), dtype=torch.float32, device=q.device)
    b, sq, hq = q.shape[0], q.shape[1], q.shape[2]
    return torch.empty((hq, b * sq), dtype=torch.float32, device=q.device).view(hq, b, sq).permute(1, 0, 2)


def _attn_fake(a):
    q = _check_attn(a, False)
    return torch.empty(q.shape, dtype=q.dtype, device=q.device)


def _attn_fwd_fake(a):
    q = _check_attn(a, True)
    return torch.empty(q.shape, dtype=q.dtype, device=q.device), _new_lse(q)


def _attn_bwd_fake(a):
    q = _check_attn(a, True)
    torch._check(a["dout"].shape == q.shape and a["out"].shape == q.shape,
                 lambda: "expected dout and out shaped like q")
    torch._check(a["lse"].dtype == torch.float32 and a["lse"].shape == _new_lse(q).shape,
                 lambda: "expected the forward's float32 lse")
    return tuple(torch.empty(t.shape, dtype=q.dtype, device=q.device) for t in (q, a["k"], a["v"]))


def _attn_bwd_sinks_fake(a):
    return (*_attn_bwd_fake(a), torch.empty((a["q"].shape[-2],), dtype=torch.float32, device=a["q"].device))


def _with_dsinks(bwd_fn):
    """bwd_fn returning four tensors whatever `sinks` is: without sinks their gradient is zeros."""
    @wraps(bwd_fn)
    def fn(*a, **kw):
        g = bwd_fn(*a, **kw)
        dq = g[0]  # q's shape
        return g if len(g) == 4 else (*g, torch.zeros((dq.shape[-2],), dtype=torch.float32, device=dq.device))
    return fn


# The table.


def _masked(packet, args, fn, fake, first="", **rest):
    """A packet's overloads over `args`: the default (or .<first>), .window and .sinks."""
    return [_Op(packet, overload, args + more, fn, fake, **rest)
            for overload, more in ((first, []), ("window", _WINDOW), ("sinks", _SINKS))]


def _attn_ops(packet, mid, fn, bwd_fn):
    """<packet> (forward only), <packet>_fwd -> (out, lse) and <packet>_bwd -> (dq, dk, dv),
    (dq, dk, dv, dsinks) from .sinks.  mid: the arguments between v / lse and causal."""
    fwd, bwd = _QKV + mid + [_NOT_CAUSAL], [_T("dout")] + _QKV + [_T("out"), _T("lse")] + mid + [_NOT_CAUSAL]
    grad = dict(as_is=_ATTN_AS_IS, forward_only=False)
    return (_masked(packet, fwd, fn, _attn_fake, as_is=_ATTN_AS_IS)
            + _masked(packet + "_fwd", fwd, partial(fn, return_lse=True), _attn_fwd_fake,
                      returns="(Tensor, Tensor)", **grad)
            + _masked(packet + "_bwd", bwd, bwd_fn, _attn_bwd_fake, returns="(Tensor, Tensor, Tensor)", **grad)[:2]
            + [_Op(packet + "_bwd", "sinks", bwd + _SINKS, _with_dsinks(bwd_fn), _attn_bwd_sinks_fake,
                   returns="(Tensor, Tensor, Tensor, Tensor)", **grad)])


_Q = [_T("q")]
_READ_TAIL = [_CAUSAL] + _SCALES
_APPEND = dict(returns="()", forward_only=False)
_ROPE_APPEND = dict(as_is=_CACHES_AS_IS, forward_only=False)
_OPS = (
    [_Op("fwd", "", _QKV + [_NOT_CAUSAL], flash_attention_fwd, _fwd_fake, as_is=())]
    + _masked("decode", _Q + _CACHE + [_KV_LENS] + _READ_TAIL, flash_attention_decode, _cache_read_fake)
    # decode_paged's pinned default has no scales: they come in .kv8, and .window / .sinks follow that
    + [_Op("decode_paged", "", _Q + _PAGES + [_KV_LENS, _CAUSAL], flash_attention_decode_paged, _cache_read_fake)]
    + _masked("decode_paged", _Q + _PAGES + [_KV_LENS] + _READ_TAIL, flash_attention_decode_paged,
              _cache_read_fake, first="kv8")
    + _masked("prefill", _Q + _CACHE + [_KV_LENS, _Q_LENS] + _READ_TAIL, flash_attention_prefill, _cache_read_fake)
    + _masked("prefill_paged", _Q + _PAGES + [_KV_LENS, _Q_LENS] + _READ_TAIL, flash_attention_prefill_paged,
              _cache_read_fake)
    + _masked("prefill_varlen", _Q + _CACHE + [_CU_Q, _KV_LENS] + _READ_TAIL, flash_attention_prefill_varlen,
              _cache_read_fake)
    + _masked("prefill_varlen_paged", _Q + _PAGES + [_CU_Q, _KV_LENS] + _READ_TAIL,
              flash_attention_prefill_varlen_paged, _cache_read_fake)
    + [_Op("cache_append", "", _NEW + _CACHE_OUT + [_T("kv_lens"), _NEW_LENS] + _SCALES,
           flash_attention_cache_append, _append_fake, **_APPEND),
       _Op("cache_append_paged", "", _NEW + _PAGES_OUT + [_T("kv_lens"), _NEW_LENS] + _SCALES,
           flash_attention_cache_append_paged, _append_fake, **_APPEND),
       _Op("cache_append_varlen", "", _NEW + _CACHE_OUT + [_CU, _T("kv_lens")] + _SCALES,
           flash_attention_cache_append_varlen, _append_fake, **_APPEND),
       _Op("cache_append_varlen_paged", "", _NEW + _PAGES_OUT + [_CU, _T("kv_lens")] + _SCALES,
           flash_attention_cache_append_varlen_paged, _append_fake, **_APPEND),
       _Op("rope_append", "", _Q + _NEW + _CACHE_OUT + [_T("kv_lens")] + _ROPE + [_NEW_LENS] + _ROPE_TAIL,
           flash_attention_rope_append, _rope_fake, **_ROPE_APPEND),
       _Op("rope_append_paged", "", _Q + _NEW + _PAGES_OUT + [_T("kv_lens")] + _ROPE + [_NEW_LENS] + _ROPE_TAIL,
           flash_attention_rope_append_paged, _rope_fake, **_ROPE_APPEND),
       _Op("rope_append_varlen", "", _Q + _NEW + _CACHE_OUT + [_CU, _T("kv_lens")] + _ROPE + _ROPE_TAIL,
           flash_attention_rope_append_varlen, _rope_fake, **_ROPE_APPEND),
       _Op("rope_append_varlen_paged", "", _Q + _NEW + _PAGES_OUT + [_CU, _T("kv_lens")] + _ROPE + _ROPE_TAIL,
           flash_attention_rope_append_varlen_paged, _rope_fake, **_ROPE_APPEND)]
    + _attn_ops("attn_varlen", [_CU_Q, _CU_K], flash_attention_varlen, flash_attention_varlen_backward)
    + _attn_ops("attn_bshd", [], flash_attention_bshd, flash_attention_bshd_backward)
)
for _op in _OPS:
    _register(_op)

fwd = torch.ops.fa_mi355x.fwd
decode = torch.ops.fa_mi355x.decode
decode_paged = torch.ops.fa_mi355x.decode_paged
prefill = torch.ops.fa_mi355x.prefill
prefill_paged = torch.ops.fa_mi355x.prefill_paged
prefill_varlen = torch.ops.fa_mi355x.prefill_varlen
prefill_varlen_paged = torch.ops.fa_mi355x.prefill_varlen_paged
cache_append = torch.ops.fa_mi355x.cache_append
cache_append_paged = torch.ops.fa_mi355x.cache_append_paged
cache_append_varlen = torch.ops.fa_mi355x.cache_append_varlen
cache_append_varlen_paged = torch.ops.fa_mi355x.cache_append_varlen_paged
rope_append = torch.ops.fa_mi355x.rope_append
rope_append_paged = torch.ops.fa_mi355x.rope_append_paged
rope_append_varlen = torch.ops.fa_mi355x.rope_append_varlen
rope_append_varlen_paged = torch.ops.fa_mi355x.rope_append_varlen_paged
attn_varlen = torch.ops.fa_mi355x.attn_varlen
attn_bshd = torch.ops.fa_mi355x.attn_bshd
attn_varlen_fwd = torch.ops.fa_mi355x.attn_varlen_fwd
attn_varlen_bwd = torch.ops.fa_mi355x.attn_varlen_bwd
attn_bshd_fwd = torch.ops.fa_mi355x.attn_bshd_fwd
attn_bshd_bwd = torch.ops.fa_mi355x.attn_bshd_bwd


# The differentiable attention: one torch.autograd.Function per layout over the
# _fwd / _bwd ops.  `sinks` is a differentiable input; its gradient is the
# backward's dsinks.


def _dout_as_given_or_dense(dout, rank):
    """dout under the stride rule as it is; otherwise contiguous -- the one
    documented copy of the backward, made here and nowhere below."""
    try:
        _token_stride(dout, "dout", rank)
    except FlashAttentionError:
        return dout.contiguous()
    return dout


def _masked_call(op, args, causal, window, sinks):
    """The default overload for a plain call, .window with only a window, else .sinks."""
    if sinks is not None:
        return op.sinks(*args, causal, window, sinks)
    return op.window(*args, causal, window) if window != 0 else op.default(*args, causal)


def _attn_forward(ctx, op, args, causal, window, sinks):
    """Saves (q, k, v, out, lse, the arguments between v and causal, sinks if given)."""
    out, lse = _masked_call(op, args, causal, window, sinks)
    ctx.save_for_backward(*args[:3], out, lse, *args[3:], *(() if sinks is None else (sinks,)))
    ctx.causal, ctx.window, ctx.has_sinks = causal, window, sinks is not None
    return out


def _attn_backward(ctx, op, dout, rank):
    """(dq, dk, dv, dsinks or None) from the overload the forward took."""
    saved = ctx.saved_tensors
    sinks, rest = (saved[-1], saved[:-1]) if ctx.has_sinks else (None, saved)
    g = _masked_call(op, (_dout_as_given_or_dense(dout, rank), *rest), ctx.causal, ctx.window, sinks)
    return g if ctx.has_sinks else (*g, None)


class _FlashAttnVarlen(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, cu_seqlens_q, cu_seqlens_k, causal, window, sinks):
        return _attn_forward(ctx, attn_varlen_fwd, (q, k, v, cu_seqlens_q, cu_seqlens_k), causal, window, sinks)

    @staticmethod
    def backward(ctx, dout):
        dq, dk, dv, dsinks = _attn_backward(ctx, attn_varlen_bwd, dout, 3)
        return dq, dk, dv, None, None, None, None, dsinks


class _FlashAttn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, causal, window, sinks):
        return _attn_forward(ctx, attn_bshd_fwd, (q, k, v), causal, window, sinks)

    @staticmethod
    def backward(ctx, dout):
        dq, dk, dv, dsinks = _attn_backward(ctx, attn_bshd_bwd, dout, 4)
        return dq, dk, dv, None, None, dsinks


def flash_attn_varlen_func(q, k, v, cu_seqlens_q, cu_seqlens_k=None, causal: bool = False, window: int = 0,
                           sinks=None):
    """Differentiable fa_mi355x.flash_attention_varlen (see fa_mi355x.flash_attn_varlen_func)."""
    return _FlashAttnVarlen.apply(q, k, v, cu_seqlens_q, cu_seqlens_k, bool(causal), window, sinks)


def flash_attn_func(q, k, v, causal: bool = False, window: int = 0, sinks=None):
    """Differentiable fa_mi355x.flash_attention_bshd (see fa_mi355x.flash_attn_func)."""
    return _FlashAttn.apply(q, k, v, bool(causal), window, sinks)
