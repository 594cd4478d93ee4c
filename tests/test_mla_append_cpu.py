"""CPU tests of the writers of the MLA caches (no GPU): fa_mi355x.MLA_APPEND_ENTRIES
against the declarations of include/fa_mi355x_mla_append.h, the C entries'
statuses in the header's order with fake pointers, the unit's kernel resources,
the torch ops' schemas and fake outputs and the Python functions' refusals."""
import ctypes
import re

import pytest
import torch

import capi_checks as cc
import fa_mi355x as fa

TYPES = {"int": ctypes.c_int, "long long": ctypes.c_longlong}
P, ODD = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x1008)
LATENT = ["fa_mla_append" + c + s + ty for c in ("", "_paged") for s in ("", "_kv8") for ty in ("_f16", "_bf16")]
INDEXER = ["fa_mla_indexer_append_k8" + c + ty for c in ("", "_paged") for ty in ("_f16", "_bf16")]
BAD, NULL, OK = fa.FA_ERR_BAD_SHAPE, fa.FA_ERR_NULL_POINTER, fa.FA_OK


def test_table_matches_the_header():
    found = re.findall(r"^([A-Za-z_][\w \*]*?)\b([a-z_][a-z0-9_]*)\s*\(([^;{]*)\)\s*;",
                       cc.header_text("fa_mi355x_mla_append.h"), re.M)
    decls = {}
    for ret, name, params in found:
        types = [re.sub(r"\s*\*\s*", "*", " ".join(re.sub(r"\b[A-Za-z_]\w*$", "", p.strip()).split()))
                 for p in params.split(",")]
        decls[name] = (TYPES[ret.strip()], [TYPES.get(t, ctypes.c_void_p) for t in types])
        assert all(t in TYPES or t.endswith("*") for t in types), (name, types)
    assert set(decls) == set(fa.MLA_APPEND_ENTRIES) == set(LATENT + INDEXER)
    assert decls == fa.MLA_APPEND_ENTRIES
    others = (fa.C_ENTRIES, fa.TREE_ENTRIES, fa.MLA_ENTRIES, fa.MLA_KV8_ENTRIES, fa.MLA_PREFILL_ENTRIES,
              fa.MLA_SPARSE_ENTRIES, fa.MLA_INDEXER_ENTRIES, fa.MLA_SPARSE_KV8_ENTRIES)
    assert not any(set(t) & set(decls) for t in others)
    syms, lib = cc.exported_symbols(), fa.load_library()
    for name, (restype, argtypes) in fa.MLA_APPEND_ENTRIES.items():
        assert name in syms, name
        assert getattr(lib, name).restype is restype and list(getattr(lib, name).argtypes) == argtypes, name


def _cache(name, cap, psz, npages, mpp, table):
    return (npages, psz, table, mpp) if "_paged" in name else (cap,)


def _latent(name, src=(P, P, P), strides=(512, 64), b=2, total=8, sn=4, cap=128, psz=64, npages=4, mpp=2, table=P,
            cu=None, lens=P, q=(P, P), hq=8, qstrides=(192 * 8, 192, 576 * 8, 576), tabs=(P, P), rope_len=16):
    tail = (None,) if "_kv8" in name else ()
    return getattr(fa.load_library(), name)(*src, *strides, b, total, sn, *_cache(name, cap, psz, npages, mpp, table),
                                            cu, lens, *q, hq, *qstrides, *tabs, rope_len, 0, None, *tail)


@pytest.mark.parametrize("name", LATENT)
def test_latent_statuses_in_order(name):
    paged, none = "_paged" in name, dict(src=(None,) * 3, table=None, lens=None, q=(None, None), tabs=(None, None))
    call = lambda **kw: _latent(name, **kw)
    for kw in (dict(hq=-1), dict(rope_len=-1), dict(b=-1), dict(total=-1), dict(total=2 ** 31 - 64)):
        assert call(**none, **kw) == BAD, kw  # sizes before everything
    if paged:
        for kw in (dict(psz=0), dict(psz=96), dict(npages=0), dict(mpp=-1), dict(psz=1 << 21), dict(mpp=1 << 26)):
            assert call(**none, b=0, **kw) == BAD, kw  # the page geometry before the empties
    else:
        assert call(**none, cap=-1) == BAD
    assert call(**none, b=0) == OK and call(**none, total=0, sn=0) == OK
    assert call(**none, sn=3) == BAD and call(**none, sn=3, cu=P) == NULL  # uniform: batch * seqlen_new == total_new
    if not paged:  # the MLA readers' capacity bound
        edge = (2 ** 31 - 1) // (576 if "_kv8" in name else 1152)
        assert call(**none, cap=edge + 1) == BAD and call(**none, cap=edge) == NULL
        assert call(**none, cap=0, hq=0) == OK  # no row and no head: nothing to do
        assert call(src=(None,) * 3, cap=0, strides=(0, 0)) != NULL  # ... no row: the cache arguments are not looked at
    for kw in (dict(strides=(511, 64)), dict(strides=(512, 72 + 4)), dict(qstrides=(192 * 8, 32, 576 * 8, 576)),
               dict(qstrides=(192 * 8, 192, 576 * 8, 580))):
        assert call(**none, **kw) == BAD, kw  # the strides before the pointers
    for i in range(3):
        assert call(src=(P,) * i + (None,) + (P,) * (2 - i), tabs=(ODD, ODD)) == NULL, i
    assert call(lens=None) == NULL and (not paged or call(table=None) == NULL)
    assert call(tabs=(P, None)) == NULL and call(tabs=(None, None)) == NULL  # heads need the tables
    assert call(q=(None, P)) == NULL and call(q=(P, None)) == NULL
    assert call(rope_len=0) == BAD and call(tabs=(ODD, P)) == BAD and call(q=(ODD, P)) == BAD
    assert call(src=(P, ODD, P)) == BAD


@pytest.mark.parametrize("name", INDEXER)
def test_indexer_statuses_in_order(name):
    paged = "_paged" in name

    def call(ptrs=(P, P, P), stride=128, b=2, total=8, sn=4, cap=128, psz=64, table=P, cu=None, lens=P):
        return getattr(fa.load_library(), name)(*ptrs, stride, b, total, sn, *_cache(name, cap, psz, 4, 2, table), cu,
                                                lens, 1, None)

    none = dict(ptrs=(None,) * 3, table=None, lens=None)
    assert call(**none, b=-1) == BAD and call(**none, total=-1) == BAD
    assert call(**none, b=0, psz=96) == (BAD if paged else OK)
    assert call(**none, total=0, sn=0) == OK and call(**none, sn=5) == BAD
    if not paged:
        assert call(**none, cap=0) == OK
    assert call(**none, stride=120) == BAD and call(**none, stride=132) == BAD
    for i in range(3):
        assert call(ptrs=(P,) * i + (None,) + (P,) * (2 - i)) == NULL, i
    assert call(lens=None) == NULL and (not paged or call(table=None) == NULL)
    assert call(ptrs=(ODD, P, P)) == BAD


def test_kernel_resource_usage():
    """Eight latent kernels (f16 / bf16 x contiguous / paged x 16-bit / FP8) and four key writers: no scratch, no LDS."""
    (kernels,) = cc.kernel_resource_usage(["fa_mla_append.hip"])
    assert len(kernels) == 12 and all(scratch == 0 and lds == 0 for _, scratch, lds in kernels), kernels


def test_ops_and_refusals():
    import fa_mi355x.torch_op_mla_append as top
    from torch._subclasses.fake_tensor import FakeTensorMode

    tail = ("Tensor? cu_seqlens=None, Tensor? q_pe=None, Tensor(b!)? q_out=None, Tensor? cos=None, Tensor? sin=None, "
            "bool interleaved=False, Tensor? ckv_scale=None) -> ()")
    assert str(top.append.default._schema) == (
        "fa_mi355x_mla::append(Tensor ckv_new, Tensor kpe_new, Tensor(a!) ckv_cache, Tensor kv_lens, " + tail)
    assert str(top.append_paged.default._schema) == (
        "fa_mi355x_mla::append_paged(Tensor ckv_new, Tensor kpe_new, Tensor(a!) ckv_pages, Tensor block_table, "
        "Tensor kv_lens, " + tail)
    assert str(top.indexer_append.default._schema) == (
        "fa_mi355x_mla::indexer_append(Tensor k_new, Tensor(a!) k_pool, Tensor kv_lens, Tensor(b!) k_scale, "
        "Tensor? cu_seqlens=None, Tensor? block_table=None, bool scale_pow2=False) -> ()")
    half = lambda *s: torch.zeros(s, dtype=torch.float16)
    lens = torch.zeros(2, dtype=torch.int32)
    with pytest.raises(ValueError, match=r"fa_mi355x_mla::append needs GPU tensors \(no CPU path\)"):
        top.append(half(4, 512), half(4, 64), half(2, 8, 576), lens)
    with pytest.raises(ValueError, match=r"fa_mi355x_mla::indexer_append needs GPU tensors"):
        top.indexer_append(half(4, 128), torch.zeros((2, 8, 128), dtype=torch.uint8), lens, torch.zeros(16))
    with FakeTensorMode():
        dev = lambda *s, dtype=torch.bfloat16: torch.empty(s, dtype=dtype, device="cuda")
        dl = dev(2, dtype=torch.int32)
        assert top.append(dev(4, 512), dev(4, 64), dev(2, 8, 576), dl) is None
        assert top.append_paged(dev(4, 512), dev(4, 64), dev(3, 64, 576, dtype=torch.uint8), dev(2, 1, dtype=torch.int32),
                                dl) is None
        assert top.indexer_append(dev(4, 128), dev(2, 8, 128, dtype=torch.uint8), dl, dev(16, dtype=torch.float32)) is None
        with pytest.raises(Exception, match="a latent cache of 576 dims"):
            top.append(dev(4, 512), dev(4, 64), dev(2, 8, 512), dl)
    # the Python functions: views are read in place, anything else is refused before the device is looked at
    app, q_out = fa.flash_attention_mla_append, half(4, 3, 576)
    good = dict(ckv_new=half(4, 512), kpe_new=half(4, 64), ckv_cache=half(2, 8, 576), kv_lens=lens)
    for match, kw in (("ckv_new must be float16 or bfloat16", dict(ckv_new=half(4, 512).float())),
                      (r"ckv_new must be \[None, 512\]", dict(ckv_new=half(4, 576))),
                      ("ckv_new must be a slice with unit inner stride", dict(ckv_new=half(512, 4).t())),
                      ("outer strides in multiples of 8", dict(kpe_new=half(4, 580)[:, 512:576])),
                      ("kpe_new must start at a multiple of 16", dict(kpe_new=half(4, 584)[:, 516:580])),
                      ("the cache must be torch.float16, torch.float8_e4m3fn", dict(ckv_cache=half(2, 8, 576).bfloat16())),
                      ("the cache must have rows of 576", dict(ckv_cache=half(2, 8, 512))),
                      ("ckv_scale goes with an FP8 cache", dict(ckv_scale=torch.ones(1))),
                      ("kv_lens must be a contiguous int32", dict(kv_lens=lens.long())),
                      ("must be 2 sequences of one length", dict(ckv_new=half(3, 512), kpe_new=half(3, 64))),
                      (r"cu_seqlens must be a contiguous int32 \[3\]", dict(cu_seqlens=lens)),
                      ("come in pairs", dict(cos=torch.zeros(8, 32))),
                      ("q_pe needs the cos and sin tables", dict(q_pe=half(4, 3, 64), q_out=q_out)),
                      ("written at Sq = 1 only", dict(q_pe=half(4, 3, 64), q_out=half(2, 3, 2, 576),
                                                      cos=torch.zeros(8, 32), sin=torch.zeros(8, 32))),
                      ("ckv_new must be a device tensor", {})):
        with pytest.raises(fa.FlashAttentionError, match=match):
            app(**{**good, **kw})
    with pytest.raises(fa.FlashAttentionError, match="k_scale must be a contiguous float32 tensor with one scale"):
        fa.flash_attention_mla_indexer_append(half(4, 128), torch.zeros((2, 8, 128), dtype=torch.uint8), lens,
                                              torch.zeros(15))
