"""CPU tests of MLA sparse attention (no GPU): fa_mi355x.MLA_SPARSE_ENTRIES
against the declarations of include/fa_mi355x_mla_sparse.h, the C entries'
statuses with fake pointers, the new unit's kernel resources and the torch op's
fake implementation.  (The float64 reference against rounding alone sits
beside the inputs it covers, unmarked, in test_mla_sparse_gpu.py: no test file
loads another.)"""
import ctypes
import re

import pytest
import torch

import capi_checks as cc
import fa_mi355x as fa

TYPES = {"int": ctypes.c_int, "float": ctypes.c_float, "unsigned long long": ctypes.c_ulonglong}
P = ctypes.c_void_p(0x1000)
NAMES = ["fa_mla_sparse_f16", "fa_mla_sparse_bf16"]


def test_table_matches_the_header():
    found = re.findall(r"^([A-Za-z_][\w \*]*?)\b([a-z_][a-z0-9_]*)\s*\(([^;{]*)\)\s*;",
                       cc.header_text("fa_mi355x_mla_sparse.h"), re.M)
    decls = {}
    for ret, name, params in found:
        types = [re.sub(r"\s*\*\s*", "*", " ".join(re.sub(r"\b[A-Za-z_]\w*$", "", p.strip()).split()))
                 for p in params.split(",")]
        decls[name] = (TYPES[ret.strip()], [TYPES.get(t, ctypes.c_void_p) for t in types])
        assert all(t in TYPES or t.endswith("*") for t in types), (name, types)
    assert set(decls) == set(fa.MLA_SPARSE_ENTRIES) == set(NAMES)
    assert decls == fa.MLA_SPARSE_ENTRIES
    others = (fa.C_ENTRIES, fa.TREE_ENTRIES, fa.MLA_ENTRIES, fa.MLA_KV8_ENTRIES, fa.MLA_PREFILL_ENTRIES)
    assert not any(set(fa.MLA_SPARSE_ENTRIES) & set(t) for t in others)
    syms, lib = cc.exported_symbols(), fa.load_library()
    for name, (restype, argtypes) in fa.MLA_SPARSE_ENTRIES.items():
        assert name in syms, name
        assert getattr(lib, name).restype is restype and list(getattr(lib, name).argtypes) == argtypes, name


def _call(name, q=P, c=P, idx=P, o=P, n=4, hq=16, topk=2048, rows=100000, scale=0.07, ns=0, ws=None, wsb=0):
    return getattr(fa.load_library(), name)(q, c, idx, o, None, n, hq, topk, rows, scale, ns, ws, wsb, None)


@pytest.mark.parametrize("name", NAMES)
def test_statuses_before_any_gpu_call(name):
    lib = fa.load_library()
    call = lambda **kw: _call(name, **kw)
    for kw in (dict(n=-1), dict(hq=-1), dict(topk=-1), dict(rows=-1), dict(ns=-1)):
        assert call(**kw) == fa.FA_ERR_BAD_SHAPE, kw
    for scale in (0.0, -0.0, -1.0, float("inf"), float("-inf"), float("nan")):
        assert call(scale=scale) == fa.FA_ERR_BAD_SHAPE, scale
        assert call(scale=scale, q=None, n=0) == fa.FA_ERR_BAD_SHAPE, scale  # a shape, before the pointers
    assert call(n=0, q=None, c=None, idx=None, o=None) == fa.FA_OK
    assert call(hq=0, q=None, c=None, idx=None, o=None) == fa.FA_OK
    assert call(n=2 ** 30, hq=2) == fa.FA_ERR_BAD_SHAPE  # N * Hq past INT_MAX
    for kw in (dict(q=None), dict(c=None), dict(idx=None), dict(o=None)):
        assert call(**kw) == fa.FA_ERR_NULL_POINTER, kw
    assert call(rows=0, o=None) == fa.FA_ERR_NULL_POINTER and call(topk=0, o=None) == fa.FA_ERR_NULL_POINTER
    # splitting needs the decode workspace: present, long enough, 16-byte aligned
    need = lib.fa_mla_decode_ws_bytes(4, 16, 1, 4)
    assert need == 65536 + 4 * 4 * 16 * 4 + 4 * 4 * 16 * 512 * 4
    assert call(ns=4) == fa.FA_ERR_WORKSPACE
    assert call(ns=4, ws=P, wsb=need - 1) == fa.FA_ERR_WORKSPACE
    assert call(ns=4, ws=ctypes.c_void_p(0x1008), wsb=need) == fa.FA_ERR_WORKSPACE
    assert lib.fa_mla_decode_num_splits(4, 16, 1, 2048) > 1 and call() == fa.FA_ERR_WORKSPACE  # the plan's own split
    assert call(ns=cc.MAX_SPLITS + 1, ws=P, wsb=1 << 40) == fa.FA_ERR_BAD_CONFIG


def test_kernel_resource_usage():
    """Four sparse kernels (f16 / bf16 x wide / narrow) beside the fill; no
    scratch, no static LDS, and the dynamic LDS the host asks for (two 72-KB
    tile images) within gfx950's 160 KB."""
    (kernels,) = cc.kernel_resource_usage(["fa_mla_sparse.hip"])
    mine = [k for k in kernels if "fa_mla_sparse_kernel" in k[0]]
    assert len(mine) == 4 and len(kernels) == 5, [k[0] for k in kernels]
    assert all(scratch == 0 and lds == 0 <= 160 * 1024 - 2 * 64 * 1152 for _, scratch, lds in kernels), kernels


def test_fake_implementation():
    import fa_mi355x.torch_op_mla_sparse as tos
    from torch._subclasses.fake_tensor import FakeTensorMode

    assert str(tos.sparse.default._schema) == ("fa_mi355x_mla::sparse(Tensor q, Tensor ckv, Tensor indices, "
                                               "float softmax_scale) -> Tensor")
    with FakeTensorMode():
        for dtype in (torch.float16, torch.bfloat16):
            pool = torch.empty((9, 64, 576), dtype=dtype, device="cuda")
            for lead in ((5,), (2, 3)):
                q = torch.empty((*lead, 128, 576), dtype=dtype, device="cuda")
                idx = torch.empty((*lead, 2048), dtype=torch.int32, device="cuda")
                o = tos.sparse(q, pool, idx, 0.1)
                assert o.shape == (*lead, 128, 512) and o.dtype == dtype and o.device.type == "cuda"
            with pytest.raises(Exception, match="int32 indices"):
                tos.sparse(q, pool, idx.long(), 0.1)
            with pytest.raises(Exception, match="softmax_scale > 0"):
                tos.sparse(q, pool, idx, 0.0)
            with pytest.raises(RuntimeError, match="forward-only"):
                tos.sparse(q.clone().requires_grad_(), pool, idx, 0.1)
    cpu = (torch.zeros((1, 1, 576), dtype=torch.float16), torch.zeros((64, 576), dtype=torch.float16),
           torch.zeros((1, 4), dtype=torch.int32))
    with pytest.raises(ValueError, match=r"fa_mi355x_mla::sparse needs GPU tensors \(no CPU path\)"):
        tos.sparse(*cpu, 0.1)
    with pytest.raises(fa.FlashAttentionError, match="softmax_scale must be finite and > 0"):
        fa.flash_attention_mla_sparse(*cpu, softmax_scale=0.0)
    with pytest.raises(fa.FlashAttentionError, match="indices must be int32"):
        fa.flash_attention_mla_sparse(cpu[0], cpu[1], cpu[2].long(), softmax_scale=0.1)
    with pytest.raises(fa.FlashAttentionError, match="ckv must be contiguous"):
        fa.flash_attention_mla_sparse(cpu[0], torch.zeros((64, 2, 576), dtype=torch.float16)[:, 0], cpu[2],
                                      softmax_scale=0.1)
    with pytest.raises(fa.FlashAttentionError, match="ckv must be torch.float16"):
        fa.flash_attention_mla_sparse(cpu[0], cpu[1].bfloat16(), cpu[2], softmax_scale=0.1)
