"""CPU tests of the fa_attn_varlen_* entries (attention over token-major Q, K
and V with no cache; no GPU): the six symbols, their argument statuses in the
header's order (all returned before any launch, so fake pointers suffice), the
Python wrappers' refusals on CPU tensors, the torch ops' schemas and fake
implementations, the uniform-mode workgroup map restated against
varlen_refs.block_of, and the compile-time resource usage of the three units.
"""
import ctypes
import re

import pytest
import torch

import attn_varlen_refs as ar
import capi_checks as cc
import fa_mi355x
import varlen_refs as vr

P = ctypes.c_void_p(0x1000)
INT_MAX = cc.INT_MAX
err = fa_mi355x.FlashAttentionError
OK, NULLP, BAD_D, BAD = (fa_mi355x.FA_OK, fa_mi355x.FA_ERR_NULL_POINTER,
                         fa_mi355x.FA_ERR_UNSUPPORTED_HEAD_DIM, fa_mi355x.FA_ERR_BAD_SHAPE)


def test_symbols_exported_and_declared():
    assert len(set(ar.SYMBOLS)) == 6
    cc.assert_exported(ar.SYMBOLS)


# ---- statuses ------------------------------------------------------------------------------

def _call(fn, variant, q=P, k=P, v=P, o=P, batch=2, hq=8, hkv=2, tq=100, tk=120, d=128, cu_q=P, cu_k=P,
          causal=1, **kw):
    return ar.call(fn, variant, q, k, v, o, None, batch, hq, hkv, tq, tk, d, cu_q, cu_k, causal, **kw)


@pytest.mark.parametrize("variant", ar.VARIANTS)
@pytest.mark.parametrize("bf16", [False, True])
def test_statuses_in_order(variant, bf16):
    """Each status with every LATER check failing too: the order of the header."""
    fn = ar.entry(fa_mi355x.load_library(), variant, bf16)
    c = lambda **kw: _call(fn, variant, **kw)  # noqa: E731
    # negative shapes first (a bad head_dim, NULL pointers and a bad stride behind them)
    for kw in (dict(batch=-1), dict(hq=-8), dict(hkv=-2), dict(tk=-1), dict(d=-128)):
        assert c(q=None, strides=(7, 0, 0), **{"d": 96, **kw}) == BAD, kw
    if variant:
        assert c(window=-1, d=96) == BAD
    # head_dim before total_q < 0, the window's causal, the strides and the modes
    for d in (0, 32, 96, 256):
        assert c(d=d, tq=-1, strides=(7, 0, 0), cu_q=None) == BAD_D
    assert c(tq=-1, q=None) == BAD
    if variant:
        assert c(window=4, causal=0, q=None) == BAD
        assert c(window=0, causal=0, q=None) == NULLP      # W = 0 needs no causal
    # strides: negative, no multiple of 8, one block's byte range past a 32-bit int
    for i in range(3):
        for s in (-8, 1027, 1028, 8 * 1024 + 4):
            st = [0, 0, 0]
            st[i] = s
            assert c(strides=tuple(st), batch=0) == BAD, (i, s)   # before the batch == 0 return
    lim_q = (INT_MAX - 256) // (127 * 2) // 8 * 8
    lim_k = (INT_MAX - 256) // (63 * 2) // 8 * 8
    assert c(strides=(lim_q, lim_k, lim_k), q=None) == NULLP
    assert c(strides=(lim_q + 8, 0, 0), q=None) == BAD
    assert c(strides=(0, lim_k + 8, 0), q=None) == BAD
    assert c(strides=(0, 0, lim_k + 8), q=None) == BAD
    # the modes
    assert c(cu_q=None, cu_k=P, batch=0) == BAD                       # cu_seqlens_k without cu_seqlens_q
    assert c(cu_q=None, cu_k=None, seqlen=(50, 61), q=None) == BAD    # total_k != B * seqlen_k
    assert c(cu_q=None, cu_k=None, seqlen=(51, 60), q=None) == BAD    # total_q != B * seqlen_q
    assert c(cu_q=None, cu_k=None, seqlen=(-50, 60), q=None) == BAD
    assert c(cu_q=None, cu_k=None, seqlen=(50, 60), q=None) == NULLP  # the uniform mode passes the shapes
    assert c(cu_q=P, cu_k=None, q=None) == NULLP                      # self-attention too
    # empty problems: FA_OK, no pointer looked at, the head counts not yet checked
    for kw in (dict(batch=0), dict(hq=0), dict(tq=0)):
        assert c(q=None, k=None, v=None, o=None, hkv=3, **kw) == OK, kw
    assert c(batch=0, cu_q=None, cu_k=None, seqlen=(0, 0), tq=0, tk=0, q=None, o=None) == OK
    # heads, a stride shorter than its heads * head_dim, the 32-bit row counts
    for hq, hkv in ((8, 3), (7, 2), (4, 8), (8, 0)):
        assert c(hq=hq, hkv=hkv, q=None) == BAD
    assert c(strides=(8 * 128 - 8, 0, 0), q=None) == BAD
    assert c(strides=(0, 2 * 128 - 8, 0), q=None) == BAD
    assert c(strides=(0, 0, 8), q=None) == BAD
    assert c(strides=(8 * 128, 2 * 128, 2 * 128 + 8), q=None) == NULLP
    assert c(tq=INT_MAX // 8 + 1, q=None) == BAD                      # heads_q * total_q
    assert c(tk=INT_MAX - 63, q=None) == BAD
    assert c(tk=INT_MAX - 64, q=None) == NULLP
    # total_k == 0: the fill needs o, and nothing else
    assert c(tk=0, o=None) == NULLP
    # NULL pointers last
    for bad in ("q", "k", "v", "o"):
        assert c(**{bad: None}) == NULLP, bad


# ---- the Python wrappers ---------------------------------------------------------------------

def _t(*shape, dtype=torch.float16):
    return torch.zeros(shape, dtype=dtype)


def test_varlen_wrapper_refusals():
    """Dtypes, ranks, views and shapes are refused before the device is looked at, so
    CPU tensors reach every message; nothing is ever copied."""
    fn = fa_mi355x.flash_attention_varlen
    q, k, cu = _t(20, 8, 64), _t(30, 2, 64), torch.zeros(4, dtype=torch.int32)
    with pytest.raises(err, match="window must be >= 0"):
        fn(q, k, k, cu, window=-1)
    with pytest.raises(err, match="a window needs causal=True"):
        fn(q, k, k, cu, window=4)
    with pytest.raises(err, match="q must be float16 or bfloat16"):
        fn(q.float(), k, k, cu)
    with pytest.raises(err, match="k must be torch.float16, got torch.bfloat16"):
        fn(q, k.bfloat16(), k, cu)
    with pytest.raises(err, match=r"q must be 3-D \[T,H,D\]"):
        fn(q[None], k, k, cu)
    with pytest.raises(err, match="out must be contiguous"):
        fn(q, k, k, cu, out=_t(20, 16, 64)[:, :8])
    with pytest.raises(err, match=r"out must be \[T,H,D\] like q"):
        fn(q, k, k, cu, out=_t(21, 8, 64))
    with pytest.raises(err, match="k and v must have one shape"):
        fn(q, k, _t(31, 2, 64), cu)
    with pytest.raises(err, match="q, k and v must agree in head_dim"):
        fn(q, _t(30, 2, 128), _t(30, 2, 128), cu)
    # views: a non-unit last stride, heads not head_dim apart, a token stride that is no multiple of 8
    with pytest.raises(err, match=r"q must have stride\(-1\) == 1 and stride\(-2\) == head_dim"):
        fn(_t(20, 8, 128)[:, :, ::2], k, k, cu)
    with pytest.raises(err, match=r"k must have stride\(-1\) == 1 and stride\(-2\) == head_dim"):
        fn(q, _t(30, 4, 64)[:, ::2], k, cu)
    with pytest.raises(err, match=r"v must have stride\(-1\) == 1"):
        fn(q, k, _t(30, 64, 2).transpose(1, 2), cu)
    odd = torch.zeros(30 * 132 + 8, dtype=torch.float16).as_strided((30, 2, 64), (132, 64, 1))
    with pytest.raises(err, match="k: the token stride 132 must be a multiple of 8 elements"):
        fn(q, odd, k, cu)
    with pytest.raises(err, match="heads_q 8 is not a multiple of heads_kv 3"):
        fn(q, _t(30, 3, 64), _t(30, 3, 64), cu)
    with pytest.raises(err, match="sinks must be a contiguous float32"):
        fn(q, k, k, cu, sinks=torch.zeros(7))
    with pytest.raises(err, match="cu_seqlens_q is required"):
        fn(q, k, k, None)
    with pytest.raises(err, match="cu_seqlens_q must be int32"):
        fn(q, k, k, cu.long())
    with pytest.raises(err, match=r"cu_seqlens_k must be a contiguous \[B \+ 1 = 4\] tensor, got \[5\]"):
        fn(q, k, k, cu, torch.zeros(5, dtype=torch.int32))
    # all of that passed: only now where the tensors live
    fused = _t(30, 12, 64)
    with pytest.raises(err, match="q must be a device tensor"):
        fn(fused[:20, :8], fused[:, 8:10], fused[:, 10:], cu, cu)
    assert fa_mi355x._token_stride(fused[:20, :8], "q", 3) == 12 * 64
    assert fa_mi355x._token_stride(q, "q", 3) == 8 * 64
    assert fa_mi355x._token_stride(q[:1], "q", 3) == 0    # one token: no stride to speak of


def test_bshd_wrapper_refusals():
    fn = fa_mi355x.flash_attention_bshd
    q, k = _t(3, 10, 8, 64), _t(3, 12, 2, 64)
    with pytest.raises(err, match=r"q must be 4-D \[B,S,H,D\]"):
        fn(q[0], k, k)
    with pytest.raises(err, match="q, k and v must agree in head_dim and batch"):
        fn(q, k[:2], k[:2])
    with pytest.raises(err, match="k: the batch stride .* is not seqlen \\* the token stride"):
        fn(q, _t(3, 24, 2, 64)[:, :12], _t(3, 24, 2, 64)[:, :12])
    with pytest.raises(err, match=r"v must have stride\(-1\) == 1 and stride\(-2\) == head_dim"):
        fn(q, k, _t(3, 2, 12, 64).transpose(1, 2))   # BHSD passed as BSHD
    with pytest.raises(err, match="a window needs causal=True"):
        fn(q, k, k, window=3)
    proj = _t(3, 10, 12 * 64)  # a fused projection output, sliced along its last dimension
    qv = proj[..., :8 * 64].unflatten(-1, (8, 64))
    assert fa_mi355x._token_stride(qv, "q", 4) == 12 * 64
    with pytest.raises(err, match="q must be a device tensor"):
        fn(qv, proj[..., 8 * 64:10 * 64].unflatten(-1, (2, 64)), proj[..., 10 * 64:].unflatten(-1, (2, 64)))


# ---- the torch ops -----------------------------------------------------------------------------

def test_ops_schemas_fake_and_cpu():
    import fa_mi355x.torch_op  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode

    ops = torch.ops.fa_mi355x
    head = "Tensor q, Tensor k, Tensor v, Tensor cu_seqlens_q, Tensor? cu_seqlens_k=None, bool causal=False"
    want = {"default": head, "window": head + ", int window=0",
            "sinks": head + ", int window=0, Tensor? sinks=None"}
    for ov, args in want.items():
        assert str(getattr(ops.attn_varlen, ov)._schema) == \
            "fa_mi355x::attn_varlen%s(%s) -> Tensor" % ("" if ov == "default" else "." + ov, args)
        assert str(getattr(ops.attn_bshd, ov)._schema) == \
            "fa_mi355x::attn_bshd%s(%s) -> Tensor" % (
                "" if ov == "default" else "." + ov,
                args.replace("Tensor cu_seqlens_q, Tensor? cu_seqlens_k=None, ", ""))
    q, k, cu = _t(20, 8, 64), _t(30, 2, 64), torch.zeros(4, dtype=torch.int32)
    with pytest.raises(ValueError, match="needs GPU tensors"):
        ops.attn_varlen(q, k, k, cu)
    with pytest.raises(ValueError, match="needs GPU tensors"):
        ops.attn_bshd(q[None], k[None], k[None], True, window=4)
    with FakeTensorMode():
        fq = torch.empty((20, 12, 64), dtype=torch.bfloat16, device="cuda")[:, :8]  # a strided view
        fk = torch.empty((30, 2, 64), dtype=torch.bfloat16, device="cuda")
        fcu = torch.empty(4, dtype=torch.int32, device="cuda")
        fs = torch.empty(8, device="cuda")
        for o in (ops.attn_varlen(fq, fk, fk, fcu), ops.attn_varlen(fq, fk, fk, fcu, fcu, True, window=5),
                  ops.attn_varlen(fq, fk, fk, fcu, causal=True, sinks=fs)):
            assert o.shape == (20, 8, 64) and o.dtype is torch.bfloat16 and o.is_contiguous()
        bq = torch.empty((3, 10, 8, 128), dtype=torch.float16, device="cuda")
        bk = torch.empty((3, 12, 2, 128), dtype=torch.float16, device="cuda")
        for o in (ops.attn_bshd(bq, bk, bk), ops.attn_bshd(bq, bk, bk, True, 4),
                  ops.attn_bshd(bq, bk, bk, sinks=fs)):
            assert o.shape == (3, 10, 8, 128) and o.dtype is torch.float16
        with pytest.raises(Exception, match="expected q"):
            ops.attn_varlen(bq, fk, fk, fcu)
        with pytest.raises(RuntimeError, match="forward-only"):
            ops.attn_varlen(fq.detach().requires_grad_(), fk, fk, fcu)


# ---- the uniform-mode map ----------------------------------------------------------------------

@pytest.mark.parametrize("bt", [128, 64])
def test_uniform_map_is_the_packed_map_on_arange_times_s(bt):
    """varlen_block_u without a cu array answers, for every virtual block id the
    host launches (and the one past them), what the packed map answers on cu =
    arange(B + 1) * S: the kernel reads i * S wherever it would read cu[i]."""
    for nseq in (1, 2, 3, 7):
        for s in (0, 1, bt - 1, bt, bt + 1, 130, 2 * bt, 3 * bt + 5):
            cu, total = [i * s for i in range(nseq + 1)], nseq * s
            ids = vr.num_ids(total, nseq, bt)
            got = [ar.block_of_uniform(nseq, s, bt, i) for i in range(ids + 1)]
            assert got == [vr.block_of(cu, total, bt, i) for i in range(ids + 1)], (nseq, s)
            want = {(b, r) for b in range(nseq) for r in range(-(-s // bt))}
            hits = [x for x in got if x is not None]
            assert set(hits) == want and len(hits) == len(want), (nseq, s)


def test_base_shape():
    assert ar.CU_Q == [0, 0, 1, 128, 256, 577] and ar.CU_K == [3, 10, 211, 311, 509, 1030]
    assert vr.spans(ar.CU_K, ar.TK) == [(3, 7), (10, 201), (211, 100), (311, 198), (509, 521)]
    off = [nk - nq for nk, nq in zip(ar.NK, ar.NQ)]
    assert off == [7, 200, -27, 70, 200]            # element 2: its first 27 rows see nothing
    assert [s % 64 for s, _ in vr.spans(ar.CU_K, ar.TK)] == [3, 10, 19, 55, 61]
    assert int(vr.owned_rows(ar.CU_K, ar.TK).sum()) == 1027 and int(vr.owned_rows(ar.CU_Q, ar.TQ).sum()) == 577


# ---- compile-time resource usage -----------------------------------------------------------------

def test_no_scratch_and_64k_lds():
    """The twelve new kernels: no scratch (no spills) and 64 KiB of LDS, as their
    packed contiguous-cache twins (fa_prefill_varlen[_win|_sink].hip, held to the
    same by their own CPU tests)."""
    units = ["fa_attn_varlen.hip", "fa_attn_varlen_win.hip", "fa_attn_varlen_sink.hip"]
    usage = cc.kernel_resource_usage(units)
    names = []
    for unit, rows in zip(units, usage):
        kernels = [r for r in rows if "fa_prefill_kernel" in r[0]]
        assert len(kernels) == 4, (unit, [r[0] for r in rows])
        for name, scratch, lds in kernels:
            assert re.search("PrefillPacked.*PrefillTokenKV", name), name
            assert scratch == 0 and lds == 65536, (unit, name, scratch, lds)
            names.append(name)
    assert len(set(names)) == 12
