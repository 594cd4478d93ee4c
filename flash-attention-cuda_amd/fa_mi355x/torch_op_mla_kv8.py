"""PyTorch custom operators for MLA decode over an FP8 (E4M3) latent cache, a
fragment of torch_op_mla.py's namespace:

    import fa_mi355x.torch_op_mla_kv8  # registers torch.ops.fa_mi355x_mla.decode_kv8 / decode_paged_kv8
    o = torch.ops.fa_mi355x_mla.decode_kv8(q, ckv8_cache, softmax_scale, ckv_scale, kv_lens)
    o = torch.ops.fa_mi355x_mla.decode_paged_kv8(q, ckv8_pages, block_table, softmax_scale, ckv_scale, kv_lens)

Two ops with one schema each,

    (q, cache | pool + block_table, float softmax_scale, ckv_scale=None, kv_lens=None, causal=True) -> Tensor

rows of torch_op.py's kind, registered by its factory under its rules, with
torch_op_mla.py's fake check: the cache (torch.float8_e4m3fn or torch.uint8)
and the scale (a float32 tensor of one element, None: 1.0) are passed as they
are.  What the arguments mean: fa_mi355x.flash_attention_mla_decode_kv8.
"""
from __future__ import annotations

import torch

from . import flash_attention_mla_decode_kv8, flash_attention_mla_decode_paged_kv8
from .torch_op import _CAUSAL, _KV_LENS, _Op, _REQUIRED, _T, _opt, _register
from .torch_op_mla import _AS_IS, _fake as _fake_mla

_LIB = torch.library.Library("fa_mi355x_mla", "FRAGMENT")

_TAIL = [("float", "softmax_scale", _REQUIRED), _opt("ckv_scale"), _KV_LENS, _CAUSAL]


def _decode_kv8(q, ckv_cache, softmax_scale, ckv_scale=None, kv_lens=None, causal=True):
    return flash_attention_mla_decode_kv8(q, ckv_cache, kv_lens, ckv_scale=ckv_scale, softmax_scale=softmax_scale,
                                          causal=causal)


def _decode_paged_kv8(q, ckv_pages, block_table, softmax_scale, ckv_scale=None, kv_lens=None, causal=True):
    return flash_attention_mla_decode_paged_kv8(q, ckv_pages, block_table, kv_lens, ckv_scale=ckv_scale,
                                                softmax_scale=softmax_scale, causal=causal)


def _fake(a):
    c = a["ckv_pages"] if "ckv_pages" in a else a["ckv_cache"]
    torch._check(c.dtype in (torch.float8_e4m3fn, torch.uint8), lambda: "expected an E4M3 (or uint8) latent cache")
    s = a["ckv_scale"]
    torch._check(s is None or (s.dtype == torch.float32 and s.numel() == 1),
                 lambda: "expected ckv_scale a float32 tensor of one element")
    return _fake_mla(a)


_KV8_AS_IS = _AS_IS | {"ckv_scale"}
_OPS = [_Op("decode_kv8", "", [_T("q"), _T("ckv_cache")] + _TAIL, _decode_kv8, _fake, as_is=_KV8_AS_IS, guard=2),
        _Op("decode_paged_kv8", "", [_T("q"), _T("ckv_pages"), _T("block_table")] + _TAIL, _decode_paged_kv8, _fake,
            as_is=_KV8_AS_IS)]
for _op in _OPS:
    _register(_op, _LIB, "fa_mi355x_mla")

decode_kv8 = torch.ops.fa_mi355x_mla.decode_kv8
decode_paged_kv8 = torch.ops.fa_mi355x_mla.decode_paged_kv8
