"""PyTorch custom operators for the MLA sparse indexer (DeepSeek-V3.2's DSA),
a fragment of torch_op_mla.py's namespace:

    import fa_mi355x.torch_op_mla_indexer  # registers the three ops below
    idx = torch.ops.fa_mi355x_mla.indexer(q, k, weights, ks, ke, topk, max_len)      # int32 [N, topk]
    o = torch.ops.fa_mi355x_mla.sparse(q_abs, ckv_pool, idx, softmax_scale)

    indexer_logits(Tensor q, Tensor k, Tensor weights, Tensor ks, Tensor ke, int max_len, Tensor? k_scale=None) -> Tensor
    indexer_topk(Tensor logits, Tensor ks, Tensor ke, int topk, int num_rows) -> Tensor
    indexer(Tensor q, Tensor k, Tensor weights, Tensor ks, Tensor ke, int topk, int max_len, Tensor? k_scale=None) -> Tensor

rows of torch_op.py's kind, registered by its factory under its rules: the CUDA
key directly, a fake implementation, no CPU path (a CPU tensor raises
ValueError), forward only, every tensor passed as it is (nothing is copied).
What the arguments mean: fa_mi355x.flash_attention_mla_indexer_logits, _topk
and flash_attention_mla_indexer.
"""
from __future__ import annotations

import torch

from . import (MLA_INDEXER_DIM, MLA_INDEXER_HEADS, flash_attention_mla_indexer, flash_attention_mla_indexer_logits,
               flash_attention_mla_indexer_topk)
from . import torch_op_mla  # noqa: F401  (defines the namespace this module is a fragment of)
from .torch_op import _Op, _REQUIRED, _T, _opt, _register

_LIB = torch.library.Library("fa_mi355x_mla", "FRAGMENT")
_QKW = [_T("q"), _T("k"), _T("weights"), _T("ks"), _T("ke")]
_AS_IS = {"q", "k", "weights", "ks", "ke", "k_scale", "logits"}


def _logits(q, k, weights, ks, ke, max_len, k_scale=None):
    return flash_attention_mla_indexer_logits(q, k, weights, ks, ke, k_scale=k_scale, max_len=max_len)


def _topk(logits, ks, ke, topk, num_rows):
    return flash_attention_mla_indexer_topk(logits, ks, ke, topk, num_rows=num_rows)


def _indexer(q, k, weights, ks, ke, topk, max_len, k_scale=None):
    return flash_attention_mla_indexer(q, k, weights, ks, ke, topk=topk, max_len=max_len, k_scale=k_scale)


def _check_qk(a):
    q, k = a["q"], a["k"]
    torch._check(q.dim() == 3 and tuple(q.shape[1:]) == (MLA_INDEXER_HEADS, MLA_INDEXER_DIM),
                 lambda: "expected q [N, %d, %d]" % (MLA_INDEXER_HEADS, MLA_INDEXER_DIM))
    torch._check(q.dtype in (torch.float16, torch.bfloat16), lambda: "expected fp16 or bf16")
    torch._check(k.dim() >= 2 and k.shape[-1] == MLA_INDEXER_DIM,
                 lambda: "expected a key pool of %d dims" % MLA_INDEXER_DIM)
    _check_ranges(a, q.shape[0])
    torch._check(a["max_len"] >= 0, lambda: "expected max_len >= 0")
    return q


def _check_ranges(a, n):
    torch._check(all(a[x].dtype == torch.int32 and tuple(a[x].shape) == (n,) for x in ("ks", "ke")),
                 lambda: "expected int32 ks and ke, one per token")


def _logits_fake(a):
    q = _check_qk(a)
    return torch.empty((q.shape[0], a["max_len"]), dtype=torch.float32, device=q.device)


def _topk_fake(a):
    lg = a["logits"]
    torch._check(lg.dim() == 2 and lg.dtype == torch.float32, lambda: "expected fp32 logits [N, max_len]")
    _check_ranges(a, lg.shape[0])
    torch._check(a["topk"] >= 0 and a["num_rows"] >= 0, lambda: "expected topk >= 0 and num_rows >= 0")
    return torch.empty((lg.shape[0], a["topk"]), dtype=torch.int32, device=lg.device)


def _indexer_fake(a):
    q = _check_qk(a)
    torch._check(a["topk"] >= 0, lambda: "expected topk >= 0")
    return torch.empty((q.shape[0], a["topk"]), dtype=torch.int32, device=q.device)


_INT = lambda name: ("int", name, _REQUIRED)  # noqa: E731
for _op in (_Op("indexer_logits", "", _QKW + [_INT("max_len"), _opt("k_scale")], _logits, _logits_fake, as_is=_AS_IS),
            _Op("indexer_topk", "", [_T("logits"), _T("ks"), _T("ke"), _INT("topk"), _INT("num_rows")], _topk,
                _topk_fake, as_is=_AS_IS),
            _Op("indexer", "", _QKW + [_INT("topk"), _INT("max_len"), _opt("k_scale")], _indexer, _indexer_fake,
                as_is=_AS_IS)):
    _register(_op, _LIB, "fa_mi355x_mla")

indexer_logits = torch.ops.fa_mi355x_mla.indexer_logits
indexer_topk = torch.ops.fa_mi355x_mla.indexer_topk
indexer = torch.ops.fa_mi355x_mla.indexer
