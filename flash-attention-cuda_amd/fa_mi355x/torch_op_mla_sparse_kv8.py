"""PyTorch custom operator for MLA sparse attention over an FP8 (E4M3) latent
pool, a fragment of torch_op_mla.py's namespace:

    import fa_mi355x.torch_op_mla_sparse_kv8  # registers torch.ops.fa_mi355x_mla.sparse_kv8
    o = torch.ops.fa_mi355x_mla.sparse_kv8(q, ckv8, indices, softmax_scale, ckv_scale)

One op with one schema,

    (Tensor q, Tensor ckv8, Tensor indices, float softmax_scale, Tensor? ckv_scale=None) -> Tensor

a row of torch_op.py's kind, registered by its factory under its rules, with
torch_op_mla_sparse.py's fake check: the pool (torch.float8_e4m3fn or
torch.uint8) and the scale (a float32 tensor of one element, None: 1.0) are
passed as they are.  What the arguments mean:
fa_mi355x.flash_attention_mla_sparse_kv8.
"""
from __future__ import annotations

import torch

from . import flash_attention_mla_sparse_kv8
from .torch_op import _Op, _REQUIRED, _T, _opt, _register
from .torch_op_mla_sparse import _fake as _fake_sparse

_LIB = torch.library.Library("fa_mi355x_mla", "FRAGMENT")


def _sparse_kv8(q, ckv8, indices, softmax_scale, ckv_scale=None):
    return flash_attention_mla_sparse_kv8(q, ckv8, indices, softmax_scale, ckv_scale)


def _fake(a):
    torch._check(a["ckv8"].dtype in (torch.float8_e4m3fn, torch.uint8),
                 lambda: "expected an E4M3 (or uint8) latent pool")
    s = a["ckv_scale"]
    torch._check(s is None or (s.dtype == torch.float32 and s.numel() == 1),
                 lambda: "expected ckv_scale a float32 tensor of one element")
    return _fake_sparse({**a, "ckv": a["ckv8"]})


_register(_Op("sparse_kv8", "", [_T("q"), _T("ckv8"), _T("indices"), ("float", "softmax_scale", _REQUIRED),
                                 _opt("ckv_scale")], _sparse_kv8, _fake, as_is={"ckv8", "ckv_scale"}),
          _LIB, "fa_mi355x_mla")

sparse_kv8 = torch.ops.fa_mi355x_mla.sparse_kv8
