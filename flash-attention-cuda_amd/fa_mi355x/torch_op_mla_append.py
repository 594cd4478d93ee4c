"""PyTorch custom operators for the writers of the MLA caches, a fragment of
torch_op_mla.py's namespace:

    import fa_mi355x.torch_op_mla_append  # registers the three ops below
    torch.ops.fa_mi355x_mla.append(ckv_new, kpe_new, ckv_cache, kv_lens, None, q_pe, q_out, cos, sin)
    o = torch.ops.fa_mi355x_mla.decode(q_out, ckv_cache, kv_lens, softmax_scale)

    append(Tensor ckv_new, Tensor kpe_new, Tensor(a!) ckv_cache, Tensor kv_lens, Tensor? cu_seqlens=None,
           Tensor? q_pe=None, Tensor(b!)? q_out=None, Tensor? cos=None, Tensor? sin=None, bool interleaved=False,
           Tensor? ckv_scale=None) -> ()
    append_paged(Tensor ckv_new, Tensor kpe_new, Tensor(a!) ckv_pages, Tensor block_table, Tensor kv_lens, ...) -> ()
    indexer_append(Tensor k_new, Tensor(a!) k_pool, Tensor kv_lens, Tensor(b!) k_scale, Tensor? cu_seqlens=None,
                   Tensor? block_table=None, bool scale_pow2=False) -> ()

rows of torch_op.py's kind, registered by its factory under its rules: the CUDA
key directly, a fake implementation, no CPU path (a CPU tensor raises
ValueError), every tensor passed as it is (nothing is copied).  The caches and
q_out are mutated arguments, as in cache_append's schema.  What the arguments
mean: fa_mi355x.flash_attention_mla_append, _append_paged and
flash_attention_mla_indexer_append.
"""
from __future__ import annotations

import torch

from . import (MLA_DQK, MLA_DV, MLA_INDEXER_DIM, flash_attention_mla_append, flash_attention_mla_append_paged,
               flash_attention_mla_indexer_append)
from . import torch_op_mla  # noqa: F401  (defines the namespace this module is a fragment of)
from .torch_op import _Op, _T, _opt, _register

_LIB = torch.library.Library("fa_mi355x_mla", "FRAGMENT")
_TAIL = [_opt("cu_seqlens"), _opt("q_pe"), ("Tensor(b!)?", "q_out", None), _opt("cos"), _opt("sin"),
         ("bool", "interleaved", False), _opt("ckv_scale")]
_AS_IS = {"ckv_new", "kpe_new", "ckv_cache", "ckv_pages", "block_table", "kv_lens", "cu_seqlens", "q_pe", "q_out",
          "cos", "sin", "ckv_scale", "k_new", "k_pool", "k_scale"}


def _append_fake(a):
    ckv, kpe = a["ckv_new"], a["kpe_new"]
    cache = a["ckv_pages"] if "ckv_pages" in a else a["ckv_cache"]
    torch._check(ckv.dim() == 2 and ckv.shape[1] == MLA_DV and tuple(kpe.shape) == (ckv.shape[0], MLA_DQK - MLA_DV),
                 lambda: "expected ckv_new [T, %d] and kpe_new [T, %d]" % (MLA_DV, MLA_DQK - MLA_DV))
    torch._check(ckv.dtype in (torch.float16, torch.bfloat16), lambda: "expected fp16 or bf16")
    torch._check(cache.dim() == 3 and cache.shape[2] == MLA_DQK, lambda: "expected a latent cache of %d dims" % MLA_DQK)
    torch._check((a["q_pe"] is None) == (a["q_out"] is None), lambda: "expected q_pe and q_out together")


def _indexer_append_fake(a):
    k, pool = a["k_new"], a["k_pool"]
    torch._check(k.dim() == 2 and k.shape[1] == MLA_INDEXER_DIM, lambda: "expected k_new [T, %d]" % MLA_INDEXER_DIM)
    torch._check(pool.dim() == 3 and pool.shape[2] == MLA_INDEXER_DIM,
                 lambda: "expected a key pool of %d dims" % MLA_INDEXER_DIM)
    torch._check(a["k_scale"].dtype == torch.float32, lambda: "expected float32 k_scale")


_NEW = [_T("ckv_new"), _T("kpe_new")]
_WRITER = dict(as_is=_AS_IS, returns="()", forward_only=False)
for _op in (_Op("append", "", _NEW + [_T("ckv_cache", "(a!)"), _T("kv_lens")] + _TAIL, flash_attention_mla_append,
                _append_fake, **_WRITER),
            _Op("append_paged", "", _NEW + [_T("ckv_pages", "(a!)"), _T("block_table"), _T("kv_lens")] + _TAIL,
                flash_attention_mla_append_paged, _append_fake, **_WRITER),
            _Op("indexer_append", "", [_T("k_new"), _T("k_pool", "(a!)"), _T("kv_lens"), _T("k_scale", "(b!)"),
                                       _opt("cu_seqlens"), _opt("block_table"), ("bool", "scale_pow2", False)],
                flash_attention_mla_indexer_append, _indexer_append_fake, **_WRITER)):
    _register(_op, _LIB, "fa_mi355x_mla")

append = torch.ops.fa_mi355x_mla.append
append_paged = torch.ops.fa_mi355x_mla.append_paged
indexer_append = torch.ops.fa_mi355x_mla.indexer_append
