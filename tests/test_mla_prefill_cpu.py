"""CPU tests of MLA prefill (no GPU): fa_mi355x.MLA_PREFILL_ENTRIES against the
declarations of include/fa_mi355x_mla_prefill.h, the C entries' statuses with
fake pointers, the new unit's kernel resources, the torch ops' schemas and fake
implementations.  (The GPU test's references against its gates:
test_mla_prefill_gpu.py's unmarked test, which runs without a GPU.)"""
import ctypes
import re
import subprocess

import pytest
import torch

import capi_checks as cc
import fa_mi355x as fa

TYPES = {"int": ctypes.c_int, "float": ctypes.c_float, "long long": ctypes.c_longlong}
P = ctypes.c_void_p(0x1000)
NAMES = ["fa_mla_prefill_varlen_f16", "fa_mla_prefill_varlen_bf16"]


def test_table_matches_the_header():
    found = re.findall(r"^([A-Za-z_][\w \*]*?)\b([a-z_][a-z0-9_]*)\s*\(([^;{]*)\)\s*;",
                       cc.header_text("fa_mi355x_mla_prefill.h"), re.M)
    decls = {}
    for ret, name, params in found:
        types = [re.sub(r"\s*\*\s*", "*", " ".join(re.sub(r"\b[A-Za-z_]\w*$", "", p.strip()).split()))
                 for p in params.split(",")]
        decls[name] = (TYPES[ret.strip()], [TYPES.get(t, ctypes.c_void_p) for t in types])
        assert all(t in TYPES or t.endswith("*") for t in types), (name, types)
    assert set(decls) == set(fa.MLA_PREFILL_ENTRIES) == set(NAMES)
    assert decls == fa.MLA_PREFILL_ENTRIES
    others = set(fa.C_ENTRIES) | set(fa.TREE_ENTRIES) | set(fa.MLA_ENTRIES) | set(fa.MLA_KV8_ENTRIES)
    assert not set(fa.MLA_PREFILL_ENTRIES) & others
    # the fa_attn_varlen_* list without head_dim, softmax_scale after causal
    attn = fa.C_ENTRIES["fa_attn_varlen_f16"][1]
    assert fa.MLA_PREFILL_ENTRIES[NAMES[0]][1] == attn[:10] + attn[11:19] + [ctypes.c_float] + attn[19:]
    syms, lib = cc.exported_symbols(), fa.load_library()
    for name, (restype, argtypes) in fa.MLA_PREFILL_ENTRIES.items():
        assert name in syms, name
        assert getattr(lib, name).restype is restype and list(getattr(lib, name).argtypes) == argtypes, name


def _call(name, q=P, k=P, v=P, o=P, b=2, hq=4, hkv=2, tq=130, tk=260, strides=(0, 0, 0), cu_q=P, cu_k=None,
          sq=0, sk=0, causal=1, scale=0.07):
    return getattr(fa.load_library(), name)(q, k, v, o, None, b, hq, hkv, tq, tk, *strides, cu_q, cu_k, sq, sk,
                                            causal, scale, None)


@pytest.mark.parametrize("name", NAMES)
def test_statuses_before_any_gpu_call(name):
    call = lambda **kw: _call(name, **kw)
    nul = dict(q=None, k=None, v=None, o=None)
    for kw in (dict(b=-1), dict(hq=-1), dict(hkv=-1), dict(tk=-1), dict(tq=-1)):
        assert call(**kw) == fa.FA_ERR_BAD_SHAPE, kw
    for scale in (0.0, -0.0, -1.0, float("inf"), float("-inf"), float("nan")):
        assert call(scale=scale) == fa.FA_ERR_BAD_SHAPE, scale
        assert call(scale=scale, b=0, **nul) == fa.FA_ERR_BAD_SHAPE, scale  # a shape, before the pointers
    assert call(cu_q=None, cu_k=P) == fa.FA_ERR_BAD_SHAPE  # cu_seqlens_k without cu_seqlens_q
    for kw in (dict(sq=65, sk=131), dict(sq=64, sk=130), dict(sq=-65, sk=130), dict(sq=65, sk=-130)):
        assert call(cu_q=None, **kw) == fa.FA_ERR_BAD_SHAPE, kw  # uniform totals that do not multiply out
    for strides in ((4 * 192 + 4, 0, 0), (0, 2 * 192 + 12, 0), (0, 0, -8),  # not multiples of 8, negative
                    (4 * 192 - 8, 0, 0), (0, 2 * 192 - 8, 0), (0, 0, 2 * 128 - 8),  # shorter than a token
                    (2 ** 31, 0, 0), (0, 0, 2 ** 31)):  # 128 / 64 rows past a 32-bit byte range
        assert call(strides=strides) == fa.FA_ERR_BAD_SHAPE, strides
    assert call(strides=(4 * 192 + 64, 2 * 192 + 8, 2 * 256), o=None) == fa.FA_ERR_NULL_POINTER  # fine strides
    assert call(hq=3, hkv=2) == fa.FA_ERR_BAD_SHAPE and call(hkv=0) == fa.FA_ERR_BAD_SHAPE
    for kw in (dict(q=None), dict(k=None), dict(v=None), dict(o=None)):
        assert call(**kw) == fa.FA_ERR_NULL_POINTER, kw
    assert call(tk=0, o=None) == fa.FA_ERR_NULL_POINTER  # rows but no keys: O is still written
    for kw in (dict(b=0), dict(hq=0), dict(tq=0), dict(b=0, cu_q=None, tq=0, tk=0, sq=5, sk=5)):
        assert call(**kw, **nul) == fa.FA_OK, kw


def test_kernel_resource_usage():
    """Two kernels (f16, bf16): no scratch and no static LDS.  The LDS is
    dynamic: the size the host asks for is the design's 80 KB (two 24-KB K and
    two 16-KB V images), half of gfx950's 160 KB, so two workgroups share a CU;
    the compiler checks the constant the launch passes against that figure."""
    (kernels,) = cc.kernel_resource_usage(["fa_mla_prefill.hip"])
    mine = [k for k in kernels if "fa_mla_prefill_kernel" in k[0]]
    assert len(mine) == 2, [k[0] for k in kernels]
    assert all(scratch == 0 and lds == 0 for _, scratch, lds in kernels), kernels
    probe = ('#include "fa_mla_prefill_kernel.hpp"\n'
             "static_assert(fa::kMlaPfLdsBytes == 2 * 64 * (384 + 256) && fa::kMlaPfLdsBytes == 81920);\n")
    res = subprocess.run([cc.HIPCC, *cc.HIPFLAGS, "-fsyntax-only", "-x", "hip", "-"], input=probe, text=True,
                         capture_output=True, timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]


def test_ops_schemas_and_fake_shapes():
    import fa_mi355x.torch_op_mla_prefill as tomp
    from torch._subclasses.fake_tensor import FakeTensorMode

    assert str(tomp.prefill_varlen.default._schema) == (
        "fa_mi355x_mla::prefill_varlen(Tensor q, Tensor k, Tensor v, float softmax_scale, Tensor? cu_seqlens_q=None, "
        "Tensor? cu_seqlens_k=None, bool causal=True, int? seqlen_q=None, int? seqlen_k=None) -> Tensor")
    assert str(tomp.prefill_bshd.default._schema) == (
        "fa_mi355x_mla::prefill_bshd(Tensor q, Tensor k, Tensor v, float softmax_scale, bool causal=True) -> Tensor")
    with FakeTensorMode():
        for dtype in (torch.float16, torch.bfloat16):
            q, k, v = (torch.empty((70, h, d), dtype=dtype, device="cuda") for h, d in ((4, 192), (2, 192), (2, 128)))
            cu = torch.empty((3,), dtype=torch.int32, device="cuda")
            for o in (tomp.prefill_varlen(q, k, v, 0.1, cu), tomp.prefill_varlen(q, k, v, 0.1, cu, cu, False),
                      tomp.prefill_varlen(q, k, v, 0.1, seqlen_q=35, seqlen_k=35)):
                assert o.shape == (70, 4, 128) and o.dtype == dtype and o.device.type == "cuda"
            o = tomp.prefill_bshd(q.unflatten(0, (2, 35)), k.unflatten(0, (2, 35)), v.unflatten(0, (2, 35)), 0.1)
            assert o.shape == (2, 35, 4, 128) and o.dtype == dtype
            with pytest.raises(Exception, match="softmax_scale > 0"):
                tomp.prefill_varlen(q, k, v, 0.0, cu)
            with pytest.raises(Exception, match="D = 128"):
                tomp.prefill_varlen(q, k, k, 0.1, cu)
            with pytest.raises(RuntimeError, match="forward-only"):
                tomp.prefill_varlen(q.clone().requires_grad_(), k, v, 0.1, cu)
    cpu = [torch.zeros((1, 1, d), dtype=torch.float16) for d in (192, 192, 128)]
    with pytest.raises(ValueError, match=r"fa_mi355x_mla::prefill_varlen needs GPU tensors \(no CPU path\)"):
        tomp.prefill_varlen(*cpu, 0.1)
    with pytest.raises(fa.FlashAttentionError, match="softmax_scale must be finite and > 0"):
        fa.flash_attention_mla_prefill_varlen(*cpu, softmax_scale=float("nan"))
    cu = torch.zeros((2,), dtype=torch.int32)
    with pytest.raises(fa.FlashAttentionError, match="not both"):
        fa.flash_attention_mla_prefill_varlen(*cpu, cu, softmax_scale=0.1, seqlen_q=1, seqlen_k=1)
    with pytest.raises(fa.FlashAttentionError, match="given together"):
        fa.flash_attention_mla_prefill_varlen(*cpu, softmax_scale=0.1, seqlen_q=1)
    kv = torch.zeros((4, 2, 256), dtype=torch.float16)  # per-head interleaved [k_nope | v]: a head stride
    with pytest.raises(fa.FlashAttentionError, match=r"stride\(-2\) == head_dim"):
        fa.flash_attention_mla_prefill_varlen(torch.zeros((4, 2, 192), dtype=torch.float16),
                                              torch.zeros((4, 2, 192), dtype=torch.float16), kv[..., 128:],
                                              torch.zeros((2,), dtype=torch.int32), softmax_scale=0.1)
    with pytest.raises(fa.FlashAttentionError, match="last dim of 192"):
        fa.flash_attention_mla_prefill_bshd(*(t[None] for t in (cpu[0], cpu[1], cpu[1])), softmax_scale=0.1)

