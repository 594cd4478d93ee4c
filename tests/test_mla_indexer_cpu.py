"""CPU tests of the MLA sparse indexer (no GPU): fa_mi355x.MLA_INDEXER_ENTRIES
against the declarations of include/fa_mi355x_mla_indexer.h, the C entries'
statuses in the header's order with fake pointers, the unit's kernel resources
and the Python functions' refusals."""
import ctypes
import re

import pytest
import torch

import capi_checks as cc
import fa_mi355x as fa

TYPES = {"int": ctypes.c_int, "long long": ctypes.c_longlong}
P = ctypes.c_void_p(0x1000)
LOGITS = ["fa_mla_indexer_logits" + k8 + ty for k8 in ("", "_k8") for ty in ("_f16", "_bf16")]


def test_table_matches_the_header():
    found = re.findall(r"^([A-Za-z_][\w \*]*?)\b([a-z_][a-z0-9_]*)\s*\(([^;{]*)\)\s*;",
                       cc.header_text("fa_mi355x_mla_indexer.h"), re.M)
    decls = {}
    for ret, name, params in found:
        types = [re.sub(r"\s*\*\s*", "*", " ".join(re.sub(r"\b[A-Za-z_]\w*$", "", p.strip()).split()))
                 for p in params.split(",")]
        decls[name] = (TYPES[ret.strip()], [TYPES.get(t, ctypes.c_void_p) for t in types])
        assert all(t in TYPES or t.endswith("*") for t in types), (name, types)
    assert set(decls) == set(fa.MLA_INDEXER_ENTRIES) == set(LOGITS + ["fa_mla_indexer_topk"])
    assert decls == fa.MLA_INDEXER_ENTRIES
    syms, lib = cc.exported_symbols(), fa.load_library()
    for name, (restype, argtypes) in fa.MLA_INDEXER_ENTRIES.items():
        assert name in syms, name
        assert getattr(lib, name).restype is restype and list(getattr(lib, name).argtypes) == argtypes, name


def _logits(name, ptrs=(P,) * 6, scale=P, n=4, heads=64, rows=1000, max_len=128, stride=128):
    tail = (scale,) if "_k8" in name else ()
    return getattr(fa.load_library(), name)(*ptrs, n, heads, rows, max_len, stride, None, *tail)


def _topk(ptrs=(P,) * 4, n=4, rows=1000, max_len=128, stride=128, topk=16):
    return fa.load_library().fa_mla_indexer_topk(*ptrs, n, rows, max_len, stride, topk, None)


@pytest.mark.parametrize("name", LOGITS)
def test_logits_statuses_in_order(name):
    call = lambda **kw: _logits(name, **kw)
    none = (None,) * 6
    for kw in (dict(n=-1), dict(heads=-1), dict(rows=-1), dict(max_len=-1), dict(stride=-1), dict(stride=127)):
        assert call(ptrs=none, **kw) == fa.FA_ERR_BAD_SHAPE, kw  # sizes before the pointers
    for heads in (0, 32, 128):
        assert call(ptrs=none, n=0, heads=heads) == fa.FA_ERR_BAD_SHAPE, heads  # ... and before zero tokens
    assert call(ptrs=none, scale=None, n=0) == fa.FA_OK
    for i in range(6):
        assert call(ptrs=(P,) * i + (None,) + (P,) * (5 - i), max_len=0, stride=0) == fa.FA_ERR_NULL_POINTER, i
    if "_k8" in name:
        assert call(scale=None, rows=0) == fa.FA_ERR_NULL_POINTER
    assert call(max_len=0) == fa.FA_OK and call(rows=0) == fa.FA_OK  # nothing to write: no launch


def test_topk_statuses_in_order():
    none = (None,) * 4
    for kw in (dict(n=-1), dict(rows=-1), dict(max_len=-1), dict(topk=-1), dict(stride=127)):
        assert _topk(ptrs=none, **kw) == fa.FA_ERR_BAD_SHAPE, kw
    assert _topk(ptrs=none, n=0) == fa.FA_OK
    for i in range(4):
        assert _topk(ptrs=(P,) * i + (None,) + (P,) * (3 - i), topk=0) == fa.FA_ERR_NULL_POINTER, i
    assert _topk(topk=0) == fa.FA_OK


def test_kernel_resource_usage():
    """Four logits kernels (f16 / bf16 x 16-bit / FP8 keys) and the selection: no scratch; the logits
    kernels' LDS is the two tile images the kernel asserts (32 KB, 16 KB for FP8), the selection's its
    histogram, pick and per-wave counts."""
    (kernels,) = cc.kernel_resource_usage(["fa_mla_indexer.hip"])
    assert len(kernels) == 5 and all(scratch == 0 for _, scratch, _ in kernels), kernels
    lds = {name: size for name, _, size in kernels}
    assert sorted(v for k, v in lds.items() if "logits_kernel" in k) == [16384, 16384, 32768, 32768], lds
    assert [v for k, v in lds.items() if "topk_kernel" in k] == [256 * 4 + 2 * 4 + 2 * 16 * 2 * 4], lds


def test_python_refusals():
    q, k = torch.zeros((2, 64, 128), dtype=torch.float16), torch.zeros((10, 128), dtype=torch.float16)
    w, ks, ke = torch.zeros((2, 64)), torch.zeros(2, dtype=torch.int32), torch.zeros(2, dtype=torch.int32)
    logits = fa.flash_attention_mla_indexer_logits
    bad = [("q must be float16 or bfloat16", dict(q=q.float())),
           (r"q must be \[N, 64, 128\]", dict(q=q[:, :32])),
           ("k must be torch.float16", dict(k=k.bfloat16())),
           ("k must be torch.float8_e4m3fn or torch.uint8", dict(k_scale=torch.ones(10))),
           ("k_scale must be float32 with one scale per pool row", dict(k=k.to(torch.uint8), k_scale=torch.ones(9))),
           ("weights must be float32", dict(weights=w.half())),
           ("k must be contiguous", dict(k=torch.zeros((10, 2, 128), dtype=torch.float16)[:, 0])),
           ("ks must be int32", dict(ks=ks.long())),
           ("ke must be a contiguous", dict(ke=ke[:1])),
           ("max_len is required", dict(max_len=None)),
           ("q must be a tensor on q's GPU", {})]
    for match, kw in bad:
        args = dict(q=q, k=k, weights=w, ks=ks, ke=ke, max_len=8)
        args.update(kw)
        with pytest.raises(fa.FlashAttentionError, match=match):
            logits(args.pop("q"), args.pop("k"), args.pop("weights"), args.pop("ks"), args.pop("ke"), **args)
    topk = fa.flash_attention_mla_indexer_topk
    lg = torch.zeros((2, 8))
    for match, a, kw in (("topk must be an int", (lg, ks, ke, -1), dict(num_rows=10)),
                         ("num_rows must be an int", (lg, ks, ke, 4), dict(num_rows=-1)),
                         ("logits must be float32", (lg.half(), ks, ke, 4), dict(num_rows=10)),
                         ("max_len 9 must lie in", (lg, ks, ke, 4), dict(num_rows=10, max_len=9)),
                         ("unit column stride", (torch.zeros((2, 16))[:, ::2], ks, ke, 4), dict(num_rows=10)),
                         ("logits must be a tensor on", (lg, ks, ke, 4), dict(num_rows=10))):
        with pytest.raises(fa.FlashAttentionError, match=match):
            topk(*a, **kw)
    import fa_mi355x.torch_op_mla_indexer as top
    from torch._subclasses.fake_tensor import FakeTensorMode

    with pytest.raises(ValueError, match=r"fa_mi355x_mla::indexer needs GPU tensors \(no CPU path\)"):
        top.indexer(q, k, w, ks, ke, 4, 8)
    with FakeTensorMode():
        dq, dk = (torch.empty(s, dtype=torch.bfloat16, device="cuda") for s in ((5, 64, 128), (3, 7, 128)))
        dw, ds = torch.empty((5, 64), device="cuda"), torch.empty(5, dtype=torch.int32, device="cuda")
        lgt = top.indexer_logits(dq, dk, dw, ds, ds, 21)
        assert lgt.shape == (5, 21) and lgt.dtype == torch.float32
        for lists in (top.indexer_topk(lgt, ds, ds, 2048, 21), top.indexer(dq, dk, dw, ds, ds, 2048, 21)):
            assert lists.shape == (5, 2048) and lists.dtype == torch.int32 and lists.device.type == "cuda"
        with pytest.raises(Exception, match="int32 ks and ke"):
            top.indexer(dq, dk, dw, ds.long(), ds, 4, 8)
