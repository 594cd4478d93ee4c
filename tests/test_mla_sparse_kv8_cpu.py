"""MLA sparse attention over an FP8 latent pool without a GPU:
MLA_SPARSE_KV8_ENTRIES against its header, statuses with fake pointers, kernel
resources, the op's schema and fake.  (The float64 reference against rounding
alone sits beside the inputs it covers, unmarked, in test_mla_sparse_kv8_gpu.py.)"""
import ctypes
import re

import pytest
import torch

import capi_checks as cc
import fa_mi355x as fa

TYPES = {"int": ctypes.c_int, "float": ctypes.c_float, "unsigned long long": ctypes.c_ulonglong}
P = ctypes.c_void_p(0x1000)
NAMES = ["fa_mla_sparse_kv8_f16", "fa_mla_sparse_kv8_bf16"]
LDS = {True: 2 * 64 * 576, False: 4 * 32 * 1024 + 4 * 64 * 8}  # wide: two 36-KB images; narrow: the merge


def test_table_matches_the_header():
    found = re.findall(r"^([A-Za-z_][\w \*]*?)\b([a-z_][a-z0-9_]*)\s*\(([^;{]*)\)\s*;",
                       cc.header_text("fa_mi355x_mla_sparse_kv8.h"), re.M)
    decls = {}
    for ret, name, params in found:
        types = [re.sub(r"\s*\*\s*", "*", " ".join(re.sub(r"\b[A-Za-z_]\w*$", "", p.strip()).split()))
                 for p in params.split(",")]
        decls[name] = (TYPES[ret.strip()], [TYPES.get(t, ctypes.c_void_p) for t in types])
        assert all(t in TYPES or t.endswith("*") for t in types), (name, types)
    assert set(decls) == set(fa.MLA_SPARSE_KV8_ENTRIES) == set(NAMES)
    assert decls == fa.MLA_SPARSE_KV8_ENTRIES
    others = (fa.C_ENTRIES, fa.TREE_ENTRIES, fa.MLA_ENTRIES, fa.MLA_KV8_ENTRIES, fa.MLA_PREFILL_ENTRIES,
              fa.MLA_SPARSE_ENTRIES, fa.MLA_INDEXER_ENTRIES)
    assert not any(set(fa.MLA_SPARSE_KV8_ENTRIES) & set(t) for t in others)
    syms, lib = cc.exported_symbols(), fa.load_library()
    for name, (restype, argtypes) in fa.MLA_SPARSE_KV8_ENTRIES.items():
        sparse = fa.MLA_SPARSE_ENTRIES[name.replace("_kv8", "")][1]
        assert name in syms and argtypes == sparse[:3] + [ctypes.c_void_p] + sparse[3:], name  # ckv_scale after indices
        assert getattr(lib, name).restype is restype and list(getattr(lib, name).argtypes) == argtypes, name


def _call(name, q=P, c=P, idx=P, sc=None, o=P, n=4, hq=16, topk=2048, rows=100000, scale=0.07, ns=0, ws=None, wsb=0):
    return getattr(fa.load_library(), name)(q, c, idx, sc, o, None, n, hq, topk, rows, scale, ns, ws, wsb, None)


@pytest.mark.parametrize("sc", [None, P], ids=["noscale", "scale"])  # NULL is 1.0: never a status, never read here
@pytest.mark.parametrize("name", NAMES)
def test_statuses_before_any_gpu_call(name, sc):
    lib = fa.load_library()
    call = lambda **kw: _call(name, sc=sc, **kw)
    for kw in (dict(n=-1), dict(hq=-1), dict(topk=-1), dict(rows=-1), dict(ns=-1)):
        assert call(**kw) == fa.FA_ERR_BAD_SHAPE, kw
    for scale in (0.0, -0.0, -1.0, float("inf"), float("-inf"), float("nan")):
        assert call(scale=scale) == fa.FA_ERR_BAD_SHAPE, scale
        assert call(scale=scale, q=None, n=0) == fa.FA_ERR_BAD_SHAPE, scale  # a shape, before the pointers
    assert call(n=0, q=None, c=None, idx=None, o=None) == call(hq=0, q=None, c=None, idx=None, o=None) == fa.FA_OK
    assert call(n=2 ** 30, hq=2) == fa.FA_ERR_BAD_SHAPE  # N * Hq past INT_MAX
    for kw in (dict(q=None), dict(c=None), dict(idx=None), dict(o=None)):
        assert call(**kw) == fa.FA_ERR_NULL_POINTER, kw
    assert call(rows=0, o=None) == fa.FA_ERR_NULL_POINTER and call(topk=0, o=None) == fa.FA_ERR_NULL_POINTER
    # splitting needs the decode workspace: present, long enough, 16-byte aligned
    need = lib.fa_mla_decode_ws_bytes(4, 16, 1, 4)
    assert call(ns=4) == call(ns=4, ws=P, wsb=need - 1) == fa.FA_ERR_WORKSPACE
    assert call(ns=4, ws=ctypes.c_void_p(0x1008), wsb=need) == fa.FA_ERR_WORKSPACE
    assert lib.fa_mla_decode_num_splits(4, 16, 1, 2048) > 1 and call() == fa.FA_ERR_WORKSPACE  # the plan's own split
    assert call(ns=cc.MAX_SPLITS + 1, ws=P, wsb=1 << 40) == fa.FA_ERR_BAD_CONFIG


def test_kernel_resource_usage():
    """Four kernels (f16 / bf16 x wide / narrow) beside the fill; no scratch, no
    static LDS, and the dynamic LDS the host asks for within gfx950's 160 KB."""
    (kernels,) = cc.kernel_resource_usage(["fa_mla_sparse_kv8.hip"])
    mine = [k for k in kernels if "fa_mla_sparse_kv8_kernel" in k[0]]
    assert len(mine) == 4 and len(kernels) == 5, [k[0] for k in kernels]
    assert sorted("Lb1E" in k[0] for k in mine) == [False, False, True, True]  # WIDE twice, narrow twice
    assert all(scratch == 0 and lds + LDS["Lb1E" in name] <= 160 * 1024 for name, scratch, lds in kernels), kernels


def test_fake_implementation():
    import fa_mi355x.torch_op_mla_sparse_kv8 as tos
    from torch._subclasses.fake_tensor import FakeTensorMode

    assert str(tos.sparse_kv8.default._schema) == ("fa_mi355x_mla::sparse_kv8(Tensor q, Tensor ckv8, Tensor indices, "
                                                   "float softmax_scale, Tensor? ckv_scale=None) -> Tensor")
    with FakeTensorMode():
        s = torch.empty((1,), dtype=torch.float32, device="cuda")
        for dtype, pdtype in ((torch.float16, torch.uint8), (torch.bfloat16, torch.float8_e4m3fn)):
            pool = torch.empty((9, 64, 576), dtype=pdtype, device="cuda")
            for lead in ((5,), (2, 3)):
                q = torch.empty((*lead, 128, 576), dtype=dtype, device="cuda")
                idx = torch.empty((*lead, 2048), dtype=torch.int32, device="cuda")
                for o in (tos.sparse_kv8(q, pool, idx, 0.1), tos.sparse_kv8(q, pool, idx, 0.1, s)):
                    assert o.shape == (*lead, 128, 512) and o.dtype == dtype and o.device.type == "cuda"
            with pytest.raises(Exception, match="E4M3"):
                tos.sparse_kv8(q, q, idx, 0.1)
            with pytest.raises(Exception, match="one element"):
                tos.sparse_kv8(q, pool, idx, 0.1, s.half())
            with pytest.raises(RuntimeError, match="forward-only"):
                tos.sparse_kv8(q.clone().requires_grad_(), pool, idx, 0.1)
    cpu = (torch.zeros((1, 1, 576), dtype=torch.float16), torch.zeros((64, 576), dtype=torch.uint8),
           torch.zeros((1, 4), dtype=torch.int32))
    with pytest.raises(ValueError, match=r"fa_mi355x_mla::sparse_kv8 needs GPU tensors \(no CPU path\)"):
        tos.sparse_kv8(*cpu, 0.1)
    with pytest.raises(fa.FlashAttentionError, match="torch.float8_e4m3fn or torch.uint8"):
        fa.flash_attention_mla_sparse_kv8(cpu[0], cpu[1].half(), cpu[2], 0.1)
    with pytest.raises(fa.FlashAttentionError, match="multiple of 16 bytes"):
        fa.flash_attention_mla_sparse_kv8(cpu[0], torch.zeros((65 * 576 + 8,), dtype=torch.uint8)[8:].view(65, 576),
                                          cpu[2], 0.1)
    with pytest.raises(fa.FlashAttentionError, match="ckv_scale must be a contiguous float32 tensor of one element"):
        fa.flash_attention_mla_sparse_kv8(*cpu, 0.1, torch.zeros((2,)))
