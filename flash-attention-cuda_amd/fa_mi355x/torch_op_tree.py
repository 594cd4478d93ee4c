"""PyTorch custom operators for the tree-masked decode (speculative-decoding
verification), in a namespace of their own beside fa_mi355x/torch_op.py's:

    import fa_mi355x.torch_op_tree  # registers torch.ops.fa_mi355x_tree.*
    mask = fa_mi355x.tree_mask_from_parents(parents)  # int32 [B, Sq]
    o = torch.ops.fa_mi355x_tree.decode(q, k_cache, v_cache, mask, kv_lens, window=128, sinks=sinks)
    o = torch.ops.fa_mi355x_tree.decode_paged(q, k_pages, v_pages, block_table, mask, kv_lens)

The schemas of ``fa_mi355x::decode`` and their overload order are pinned as
they stand, and ``tree_mask`` is no trailing argument of theirs (there is no
``causal``: the mask replaces the causal rule), so these are two ops with one
schema each,

    (q, caches | pools + block_table, tree_mask, kv_lens=None, k_scale=None,
     v_scale=None, window=0, sinks=None) -> Tensor

rows of the same kind as torch_op.py's table and registered by its factory
under its rules: the CUDA key directly, a fake implementation, no CPU path (a
CPU tensor raises ValueError), forward only, caches and pools passed as they
are.  What the arguments mean: fa_mi355x.flash_attention_decode.
"""
from __future__ import annotations

import torch

from . import flash_attention_decode, flash_attention_decode_paged
from .torch_op import (_CACHE, _KV_LENS, _PAGES, _Q, _SCALES, _SINKS, _Op, _T, _cache_read_fake,
                       _register)

_LIB = torch.library.Library("fa_mi355x_tree", "DEF")

_TAIL = [_T("tree_mask"), _KV_LENS] + _SCALES + _SINKS


def _decode(q, k_cache, v_cache, tree_mask, kv_lens=None, k_scale=None, v_scale=None, window=0, sinks=None):
    return flash_attention_decode(q, k_cache, v_cache, kv_lens, k_scale=k_scale, v_scale=v_scale,
                                  window=window, sinks=sinks, tree_mask=tree_mask)


def _decode_paged(q, k_pages, v_pages, block_table, tree_mask, kv_lens=None, k_scale=None, v_scale=None,
                  window=0, sinks=None):
    return flash_attention_decode_paged(q, k_pages, v_pages, block_table, kv_lens, k_scale=k_scale,
                                        v_scale=v_scale, window=window, sinks=sinks, tree_mask=tree_mask)


def _fake(a):
    torch._check(a["tree_mask"].dim() == 2, lambda: "expected a [B, Sq] tree_mask")
    return _cache_read_fake(a)


_OPS = [_Op("decode", "", _Q + _CACHE + _TAIL, _decode, _fake),
        _Op("decode_paged", "", _Q + _PAGES + _TAIL, _decode_paged, _fake)]
for _op in _OPS:
    _register(_op, _LIB, "fa_mi355x_tree")

decode = torch.ops.fa_mi355x_tree.decode
decode_paged = torch.ops.fa_mi355x_tree.decode_paged
