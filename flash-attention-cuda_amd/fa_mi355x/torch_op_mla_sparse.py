"""PyTorch custom operator for MLA sparse attention (top-k latent rows per
query token, DeepSeek-V3.2's DSA), a fragment of torch_op_mla.py's namespace:

    import fa_mi355x.torch_op_mla_sparse  # registers torch.ops.fa_mi355x_mla.sparse
    o = torch.ops.fa_mi355x_mla.sparse(q, ckv, indices, softmax_scale)   # q's leading shape + [512]

One op with one schema,

    (Tensor q, Tensor ckv, Tensor indices, float softmax_scale) -> Tensor

a row of torch_op.py's kind, registered by its factory under its rules: the
CUDA key directly, a fake implementation, no CPU path (a CPU tensor raises
ValueError), forward only, the pool passed as it is (it is never copied).
What the arguments mean: fa_mi355x.flash_attention_mla_sparse.
"""
from __future__ import annotations

import torch

from . import MLA_DQK, MLA_DV, flash_attention_mla_sparse
from . import torch_op_mla  # noqa: F401  (defines the namespace this module is a fragment of)
from .torch_op import _Op, _REQUIRED, _T, _register

_LIB = torch.library.Library("fa_mi355x_mla", "FRAGMENT")


def _sparse(q, ckv, indices, softmax_scale):
    return flash_attention_mla_sparse(q, ckv, indices, softmax_scale=softmax_scale)


def _fake(a):
    q, ckv, idx = a["q"], a["ckv"], a["indices"]
    torch._check(q.dim() in (3, 4) and q.shape[-1] == MLA_DQK,
                 lambda: "expected q [N, Hq, %d] or [B, Sq, Hq, %d]" % (MLA_DQK, MLA_DQK))
    torch._check(q.dtype in (torch.float16, torch.bfloat16), lambda: "expected fp16 or bf16")
    torch._check(ckv.dim() >= 2 and ckv.shape[-1] == MLA_DQK, lambda: "expected a latent pool of %d dims" % MLA_DQK)
    torch._check(idx.dtype == torch.int32 and idx.dim() == q.dim() - 1 and idx.shape[:-1] == q.shape[:-2],
                 lambda: "expected int32 indices, one list per token of q")
    torch._check(a["softmax_scale"] > 0, lambda: "expected softmax_scale > 0")
    return torch.empty((*q.shape[:-1], MLA_DV), dtype=q.dtype, device=q.device)


_register(_Op("sparse", "", [_T("q"), _T("ckv"), _T("indices"), ("float", "softmax_scale", _REQUIRED)], _sparse,
              _fake, as_is={"ckv"}), _LIB, "fa_mi355x_mla")

sparse = torch.ops.fa_mi355x_mla.sparse
