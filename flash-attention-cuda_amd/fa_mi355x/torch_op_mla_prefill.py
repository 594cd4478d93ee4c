"""PyTorch custom operators for MLA prefill (192-dim Q/K, 128-dim V, the
caller's softmax scale, no cache), a fragment of torch_op_mla.py's namespace:

    import fa_mi355x.torch_op_mla_prefill  # registers torch.ops.fa_mi355x_mla.prefill_varlen / prefill_bshd
    o = torch.ops.fa_mi355x_mla.prefill_varlen(q, k, v, softmax_scale, cu_seqlens_q)  # [T,Hq,128]
    o = torch.ops.fa_mi355x_mla.prefill_bshd(q, k, v, softmax_scale)                  # [B,Sq,Hq,128]

Two ops with one schema each,

    prefill_varlen(q, k, v, float softmax_scale, cu_seqlens_q=None, cu_seqlens_k=None, causal=True,
                   seqlen_q=None, seqlen_k=None) -> Tensor
    prefill_bshd(q, k, v, float softmax_scale, causal=True) -> Tensor

rows of torch_op.py's kind, registered by its factory under its rules: the
CUDA key directly, a fake implementation, no CPU path (a CPU tensor raises
ValueError), forward only; q, k and v are passed as they are (a token-major
view is read in place, any other layout raises).  What the arguments mean:
fa_mi355x.flash_attention_mla_prefill_varlen.
"""
from __future__ import annotations

import torch

from . import MLA_PREFILL_DQK, MLA_PREFILL_DV, flash_attention_mla_prefill_bshd, flash_attention_mla_prefill_varlen
from . import torch_op_mla  # noqa: F401  (defines the namespace this fragment extends)
from .torch_op import _ATTN_AS_IS, _CAUSAL, _Op, _QKV, _REQUIRED, _opt, _register

_LIB = torch.library.Library("fa_mi355x_mla", "FRAGMENT")

_SCALE = [("float", "softmax_scale", _REQUIRED)]


def _prefill_varlen(q, k, v, softmax_scale, cu_seqlens_q=None, cu_seqlens_k=None, causal=True, seqlen_q=None,
                    seqlen_k=None):
    return flash_attention_mla_prefill_varlen(q, k, v, cu_seqlens_q, cu_seqlens_k, softmax_scale=softmax_scale,
                                              causal=causal, seqlen_q=seqlen_q, seqlen_k=seqlen_k)


def _prefill_bshd(q, k, v, softmax_scale, causal=True):
    return flash_attention_mla_prefill_bshd(q, k, v, softmax_scale=softmax_scale, causal=causal)


def _fake(a):
    q, k, v = a["q"], a["k"], a["v"]
    rank, layout = (3, "[T, H, D]") if "cu_seqlens_q" in a else (4, "[B, S, H, D]")
    torch._check(q.dim() == rank and q.shape[-1] == MLA_PREFILL_DQK,
                 lambda: "expected q %s with D = %d" % (layout, MLA_PREFILL_DQK))
    torch._check(k.dim() == rank and k.shape[-1] == MLA_PREFILL_DQK and v.dim() == rank
                 and v.shape[-1] == MLA_PREFILL_DV,
                 lambda: "expected k %s with D = %d and v with D = %d" % (layout, MLA_PREFILL_DQK, MLA_PREFILL_DV))
    torch._check(q.dtype in (torch.float16, torch.bfloat16), lambda: "expected fp16 or bf16")
    torch._check(a["softmax_scale"] > 0, lambda: "expected softmax_scale > 0")
    cu = a.get("cu_seqlens_q")
    torch._check(cu is None or cu.dim() == 1, lambda: "expected a [B + 1] cu_seqlens_q")
    return torch.empty((*q.shape[:-1], MLA_PREFILL_DV), dtype=q.dtype, device=q.device)


_OPS = [_Op("prefill_varlen", "", _QKV + _SCALE + [_opt("cu_seqlens_q"), _opt("cu_seqlens_k"), _CAUSAL,
                                                  ("int?", "seqlen_q", None), ("int?", "seqlen_k", None)],
            _prefill_varlen, _fake, as_is=_ATTN_AS_IS),
        _Op("prefill_bshd", "", _QKV + _SCALE + [_CAUSAL], _prefill_bshd, _fake, as_is=_ATTN_AS_IS)]
for _op in _OPS:
    _register(_op, _LIB, "fa_mi355x_mla")

prefill_varlen = torch.ops.fa_mi355x_mla.prefill_varlen
prefill_bshd = torch.ops.fa_mi355x_mla.prefill_bshd
