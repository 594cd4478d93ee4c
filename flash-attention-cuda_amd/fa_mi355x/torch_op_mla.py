"""PyTorch custom operators for MLA decode (attention over a latent K/V cache),
in a namespace of their own beside fa_mi355x/torch_op.py's:

    import fa_mi355x.torch_op_mla  # registers torch.ops.fa_mi355x_mla.*
    o = torch.ops.fa_mi355x_mla.decode(q, ckv_cache, softmax_scale, kv_lens)       # [B,Hq,Sq,512]
    o = torch.ops.fa_mi355x_mla.decode_paged(q, ckv_pages, block_table, softmax_scale, kv_lens)

Two ops with one schema each,

    (q, cache | pool + block_table, float softmax_scale, kv_lens=None, causal=True) -> Tensor

rows of the same kind as torch_op.py's table and registered by its factory
under its rules: the CUDA key directly, a fake implementation, no CPU path (a
CPU tensor raises ValueError), forward only, the cache and the pool passed as
they are.  ``softmax_scale`` has no default: none would be right for every
model.  What the arguments mean: fa_mi355x.flash_attention_mla_decode.
"""
from __future__ import annotations

import torch

from . import MLA_DQK, MLA_DV, flash_attention_mla_decode, flash_attention_mla_decode_paged
from .torch_op import _CAUSAL, _KV_LENS, _Op, _REQUIRED, _T, _check_block_table, _register

_LIB = torch.library.Library("fa_mi355x_mla", "DEF")

_TAIL = [("float", "softmax_scale", _REQUIRED), _KV_LENS, _CAUSAL]


def _decode(q, ckv_cache, softmax_scale, kv_lens=None, causal=True):
    return flash_attention_mla_decode(q, ckv_cache, kv_lens, softmax_scale=softmax_scale, causal=causal)


def _decode_paged(q, ckv_pages, block_table, softmax_scale, kv_lens=None, causal=True):
    return flash_attention_mla_decode_paged(q, ckv_pages, block_table, kv_lens, softmax_scale=softmax_scale,
                                            causal=causal)


def _fake(a):
    q = a["q"]
    torch._check(q.dim() == 4 and q.shape[-1] == MLA_DQK, lambda: "expected q [B, Hq, Sq, %d]" % MLA_DQK)
    torch._check(q.dtype in (torch.float16, torch.bfloat16), lambda: "expected fp16 or bf16")
    c = a["ckv_pages"] if "ckv_pages" in a else a["ckv_cache"]
    torch._check(c.dim() == 3 and c.shape[-1] == MLA_DQK, lambda: "expected a 3-D latent cache of %d dims" % MLA_DQK)
    torch._check(a["softmax_scale"] > 0, lambda: "expected softmax_scale > 0")
    _check_block_table(a)
    return torch.empty((*q.shape[:-1], MLA_DV), dtype=q.dtype, device=q.device)


_AS_IS = {"ckv_cache", "ckv_pages"}
_OPS = [_Op("decode", "", [_T("q"), _T("ckv_cache")] + _TAIL, _decode, _fake, as_is=_AS_IS, guard=2),
        _Op("decode_paged", "", [_T("q"), _T("ckv_pages"), _T("block_table")] + _TAIL, _decode_paged, _fake,
            as_is=_AS_IS)]
for _op in _OPS:
    _register(_op, _LIB, "fa_mi355x_mla")

decode = torch.ops.fa_mi355x_mla.decode
decode_paged = torch.ops.fa_mi355x_mla.decode_paged
