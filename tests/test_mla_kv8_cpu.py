"""MLA decode over an FP8 latent cache without a GPU: MLA_KV8_ENTRIES against its
header, statuses with fake pointers, kernel resources, the ops' schemas and fakes."""
import ctypes
import re

import pytest
import torch

import capi_checks as cc
import fa_mi355x as fa

TYPES = {"int": ctypes.c_int, "float": ctypes.c_float, "unsigned long long": ctypes.c_ulonglong}
P = ctypes.c_void_p(0x1000)
NAMES = ["fa_mla_decode%s_kv8_%s" % (f, ty) for f in ("", "_paged") for ty in ("f16", "bf16")]
LDS = 4 * 64 * 576  # the dynamic LDS the host requests: a ring of four 36-KB tile images


def test_table_matches_the_header():
    found = re.findall(r"^([A-Za-z_][\w \*]*?)\b([a-z_][a-z0-9_]*)\s*\(([^;{]*)\)\s*;",
                       cc.header_text("fa_mi355x_mla_kv8.h"), re.M)
    decls = {}
    for ret, name, params in found:
        types = [re.sub(r"\s*\*\s*", "*", " ".join(re.sub(r"\b[A-Za-z_]\w*$", "", p.strip()).split()))
                 for p in params.split(",")]
        decls[name] = (TYPES[ret.strip()], [TYPES.get(t, ctypes.c_void_p) for t in types])
        assert all(t in TYPES or t.endswith("*") for t in types), (name, types)
    assert set(decls) == set(fa.MLA_KV8_ENTRIES) == set(NAMES)
    assert decls == fa.MLA_KV8_ENTRIES
    assert not set(fa.MLA_KV8_ENTRIES) & (set(fa.C_ENTRIES) | set(fa.TREE_ENTRIES) | set(fa.MLA_ENTRIES))
    syms, lib = cc.exported_symbols(), fa.load_library()
    for name, (restype, argtypes) in fa.MLA_KV8_ENTRIES.items():
        assert name in syms, name
        assert argtypes == fa.MLA_ENTRIES[name.replace("_kv8", "")][1] + [ctypes.c_void_p], name  # then ckv_scale
        assert getattr(lib, name).restype is restype and list(getattr(lib, name).argtypes) == argtypes, name


def _call(name, q=P, c=P, o=P, b=1, hq=16, sq=1, cap=4096, npages=100, psz=128, table=P, causal=1,
          scale=0.07, ns=0, ws=None, wsb=0, ckv_scale=None):
    cache = [npages, psz, table, cap // 128] if "paged" in name else [cap]
    return getattr(fa.load_library(), name)(q, c, o, None, b, hq, sq, *cache, None, causal, scale, ns, ws, wsb, None,
                                            ckv_scale)


@pytest.mark.parametrize("name", NAMES)
def test_statuses_before_any_gpu_call(name):
    lib, call = fa.load_library(), lambda **kw: _call(name, **kw)
    for kw in (dict(b=-1), dict(hq=-1), dict(ns=-1), dict(sq=0), dict(sq=17), dict(sq=-1)):
        assert call(**kw) == fa.FA_ERR_BAD_SHAPE, kw
    for scale in (0.0, -0.0, -1.0, float("inf"), float("-inf"), float("nan")):
        assert call(scale=scale) == fa.FA_ERR_BAD_SHAPE, scale
        assert call(scale=scale, q=None, b=0) == fa.FA_ERR_BAD_SHAPE, scale  # a shape, before the pointers
    for kw in (dict(q=None), dict(c=None), dict(o=None)):
        assert call(**kw) == call(ckv_scale=P, **kw) == fa.FA_ERR_NULL_POINTER, kw
    for ckv_scale in (None, P):  # NULL is 1.0: never a status, and the scale is not read on the host
        assert call(b=0, q=None, c=None, o=None, table=None, ckv_scale=ckv_scale) == fa.FA_OK
        assert call(hq=0, q=None, c=None, o=None, table=None, ckv_scale=ckv_scale) == fa.FA_OK
        assert call(ns=4, ckv_scale=ckv_scale) == fa.FA_ERR_WORKSPACE  # past every check but the workspace's
    if "paged" in name:
        for psz in (0, 32, 96, -64, 65):
            assert call(psz=psz) == fa.FA_ERR_BAD_SHAPE, psz
            assert call(psz=psz, b=0) == fa.FA_ERR_BAD_SHAPE, psz  # the page geometry is still checked
        assert call(npages=0) == fa.FA_ERR_BAD_SHAPE
        assert call(table=None) == fa.FA_ERR_NULL_POINTER
    else:
        assert call(cap=-5) == fa.FA_ERR_BAD_SHAPE
        assert call(cap=cc.INT_MAX // 576 + 1) == fa.FA_ERR_BAD_SHAPE  # cap * 576 past INT_MAX
        assert call(cap=cc.INT_MAX // 1152 + 1, ns=4) == fa.FA_ERR_WORKSPACE  # a row is 576 B, not 1152
        assert call(cap=3, sq=4) == fa.FA_ERR_BAD_SHAPE  # no kv_lens, causal, fewer rows than tokens
    # the 16-bit entries' plan and workspace: present, long enough, 16-byte aligned
    need = lib.fa_mla_decode_ws_bytes(1, 16, 1, 4)
    assert call(ns=4, ws=P, wsb=need - 1) == fa.FA_ERR_WORKSPACE
    assert call(ns=4, ws=ctypes.c_void_p(0x1008), wsb=need) == fa.FA_ERR_WORKSPACE
    assert lib.fa_mla_decode_num_splits(1, 16, 1, 4096) > 1 and call() == fa.FA_ERR_WORKSPACE  # the plan's own split
    assert call(ns=cc.MAX_SPLITS + 1, ws=P, wsb=1 << 40) == fa.FA_ERR_BAD_CONFIG


def test_kernel_resource_usage():
    """Per unit four kv8 kernels beside the fill; no scratch; static LDS + the ring within 160 KB."""
    for unit, kernels in zip(("contig", "paged"),
                             cc.kernel_resource_usage(["fa_mla_decode_kv8.hip", "fa_mla_decode_paged_kv8.hip"])):
        mine = [k for k in kernels if "fa_mla_decode_kv8_kernel" in k[0]]
        assert len(mine) == 4 and len(kernels) == 5, (unit, [k[0] for k in kernels])
        assert all(("DecodePagedKv8Params" in k[0]) == (unit == "paged") for k in mine), unit
        assert all(scratch == 0 and lds + LDS <= 160 * 1024 for _, scratch, lds in kernels), (unit, kernels)


def test_fake_implementations():
    import fa_mi355x.torch_op_mla_kv8 as tom
    from torch._subclasses.fake_tensor import FakeTensorMode

    assert str(tom.decode_kv8.default._schema) == (
        "fa_mi355x_mla::decode_kv8(Tensor q, Tensor ckv_cache, float softmax_scale, Tensor? ckv_scale=None, "
        "Tensor? kv_lens=None, bool causal=True) -> Tensor")
    assert str(tom.decode_paged_kv8.default._schema) == (
        "fa_mi355x_mla::decode_paged_kv8(Tensor q, Tensor ckv_pages, Tensor block_table, float softmax_scale, "
        "Tensor? ckv_scale=None, Tensor? kv_lens=None, bool causal=True) -> Tensor")
    with FakeTensorMode():
        for dtype in (torch.float16, torch.bfloat16):
            q = torch.empty((2, 128, 2, 576), dtype=dtype, device="cuda")
            c = torch.empty((2, 256, 576), dtype=torch.float8_e4m3fn, device="cuda")
            pool = torch.empty((9, 64, 576), dtype=torch.uint8, device="cuda")
            table = torch.empty((2, 4), dtype=torch.int32, device="cuda")
            lens = torch.empty((2,), dtype=torch.int32, device="cuda")
            s = torch.empty((1,), dtype=torch.float32, device="cuda")
            for o in (tom.decode_kv8(q, c, 0.1), tom.decode_kv8(q, c, 0.1, s, lens, False),
                      tom.decode_paged_kv8(q, pool, table, 0.1), tom.decode_paged_kv8(q, pool, table, 0.1, s, lens)):
                assert o.shape == (2, 128, 2, 512) and o.dtype == dtype and o.device.type == "cuda"
            with pytest.raises(Exception, match="softmax_scale > 0"):
                tom.decode_kv8(q, c, 0.0)
            with pytest.raises(Exception, match="E4M3"):
                tom.decode_kv8(q, q, 0.1)
    q, c = torch.zeros((1, 1, 1, 576), dtype=torch.float16), torch.zeros((1, 64, 576), dtype=torch.uint8)
    with pytest.raises(ValueError, match=r"fa_mi355x_mla::decode_kv8 needs GPU tensors \(no CPU path\)"):
        tom.decode_kv8(q, c, 0.1)
    with pytest.raises(fa.FlashAttentionError, match="torch.float8_e4m3fn or torch.uint8"):
        fa.flash_attention_mla_decode_kv8(q, c.half(), softmax_scale=0.1)
