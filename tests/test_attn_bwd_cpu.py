"""CPU tests of the backward pass of the token-major attention (no GPU): the two
symbols, the compile-time resource usage of the two new units, the C entries'
argument statuses in the header's order (all returned before any launch, so
fake pointers suffice), the torch ops' schemas, fake implementations and CPU
refusals, the references against a hand-computed case, the gate's own sanity
on the base shape, and the dK/dV kernel's key-block map restated.
"""
import ctypes
import math

import pytest
import torch

import attn_bwd_refs as br
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
    cc.assert_exported(br.SYMBOLS)


def test_no_scratch_and_lds_within_the_cu():
    """Three kernels (delta, dK/dV, dQ) x two head_dims per unit: no scratch (no
    spills), the two LDS images (+ the row constants) far inside a CU's 160 KiB."""
    units = ["fa_attn_bwd.hip", "fa_attn_bwd_bf16.hip"]
    names = []
    for unit, rows in zip(units, cc.kernel_resource_usage(units)):
        assert len(rows) == 6, (unit, [r[0] for r in rows])
        for kind, lds_want in (("delta", 0), ("dkdv", 2 * 64 * 256 + 512), ("dq", 2 * 64 * 256)):
            kernels = [r for r in rows if "fa_attn_bwd_%s_kernel" % kind in r[0]]
            assert len(kernels) == 2, (unit, kind)
            for name, scratch, lds in kernels:
                assert scratch == 0 and lds == lds_want <= 160 * 1024, (unit, name, scratch, lds)
                names.append(name)
    assert len(set(names)) == 12


# ---- statuses ------------------------------------------------------------------------------

def _call(fn, dout=P, q=P, k=P, v=P, out=P, lse=P, dq=P, dk=P, dv=P, delta=P, batch=2, hq=8, hkv=2, tq=100,
          tk=120, d=128, cu_q=P, cu_k=P, causal=1, **kw):
    return br.call(fn, dout, q, k, v, out, lse, dq, dk, dv, delta, batch, hq, hkv, tq, tk, d, cu_q, cu_k,
                   causal, **kw)


@pytest.mark.parametrize("bf16", [False, True])
def test_statuses_in_order(bf16):
    """Each status with every LATER check failing too: attn_varlen_entry's order."""
    fn = br.entry(fa_mi355x.load_library(), bf16)
    c = lambda **kw: _call(fn, **kw)  # noqa: E731
    for kw in (dict(batch=-1), dict(hq=-8), dict(hkv=-2), dict(tk=-1), dict(d=-128)):
        assert c(q=None, strides=(7, 0, 0, 0), **{"d": 96, **kw}) == BAD, kw
    for d in (0, 32, 96, 256):
        assert c(d=d, tq=-1, strides=(7, 0, 0, 0), cu_q=None) == BAD_D
    assert c(tq=-1, q=None) == BAD
    # strides (dout's first): negative, no multiple of 8, a block's byte range past a 32-bit int
    for i in range(4):
        for s in (-8, 1027, 1028, 8 * 1024 + 4):
            st = [0, 0, 0, 0]
            st[i] = s
            assert c(strides=tuple(st), batch=0) == BAD, (i, s)   # before the batch == 0 return
    lim = (INT_MAX - 256) // (127 * 2) // 8 * 8   # 128 rows of every strided tensor here
    assert c(strides=(lim, lim, lim, lim), q=None) == NULLP
    for i in range(4):
        st = [0, 0, 0, 0]
        st[i] = lim + 8
        assert c(strides=tuple(st), q=None) == BAD, i
    # the modes
    assert c(cu_q=None, cu_k=P, batch=0) == BAD
    assert c(cu_q=None, cu_k=None, seqlen=(50, 61), q=None) == BAD
    assert c(cu_q=None, cu_k=None, seqlen=(51, 60), q=None) == BAD
    assert c(cu_q=None, cu_k=None, seqlen=(-50, 60), q=None) == BAD
    assert c(cu_q=None, cu_k=None, seqlen=(50, 60), q=None) == NULLP
    assert c(cu_q=P, cu_k=None, q=None) == NULLP
    # empty problems.  Zero query heads: FA_OK, nothing looked at
    assert c(hq=0, hkv=3, dout=None, q=None, k=None, v=None, out=None, lse=None, dq=None, dk=None, dv=None,
             delta=None) == OK
    # no sequence or no query row: only dk / dv are looked at (zero-filled), the head counts not yet
    nothing = dict(dout=None, q=None, k=None, v=None, out=None, lse=None, dq=None, delta=None)
    for kw in (dict(batch=0), dict(tq=0)):
        assert c(**nothing, dk=None, hkv=3, **kw) == NULLP, kw
        assert c(**nothing, dv=None, hkv=3, **kw) == NULLP, kw
        assert c(**nothing, dk=None, dv=None, hkv=3, tk=0, **kw) == OK, kw   # ... and no key row: nothing
        assert c(**nothing, dk=None, dv=None, hkv=0, **kw) == OK, kw
    assert c(batch=0, cu_q=None, cu_k=None, seqlen=(0, 0), tq=0, tk=0, **nothing, dk=None, dv=None) == OK
    # heads, a stride shorter than its heads * head_dim, the 32-bit row counts
    for hq, hkv in ((8, 3), (7, 2), (4, 8), (8, 0)):
        assert c(hq=hq, hkv=hkv, q=None) == BAD
    assert c(strides=(8 * 128 - 8, 0, 0, 0), q=None) == BAD
    assert c(strides=(0, 8 * 128 - 8, 0, 0), q=None) == BAD
    assert c(strides=(0, 0, 2 * 128 - 8, 0), q=None) == BAD
    assert c(strides=(0, 0, 0, 8), q=None) == BAD
    assert c(strides=(8 * 128, 8 * 128 + 8, 2 * 128, 2 * 128 + 8), q=None) == NULLP
    assert c(tq=INT_MAX // 8 + 1, q=None) == BAD
    assert c(tk=INT_MAX - 63, q=None) == BAD
    assert c(tk=INT_MAX - 64, q=None) == NULLP
    # total_k == 0: the fill needs dq, and nothing else
    assert c(tk=0, dq=None) == NULLP
    # NULL pointers last, lse and delta among them
    for bad in ("dout", "q", "k", "v", "out", "lse", "dq", "dk", "dv", "delta"):
        assert c(**{bad: None}) == NULLP, bad


# ---- the Python wrappers and the torch ops -----------------------------------------------------

def _t(*shape, dtype=torch.float16):
    return torch.zeros(shape, dtype=dtype)


def test_wrapper_refusals():
    """Refused before the device is looked at, so CPU tensors reach every message."""
    fn = fa_mi355x.flash_attention_varlen_backward
    q, k, cu = _t(20, 8, 64), _t(30, 2, 64), torch.zeros(4, dtype=torch.int32)
    lse = torch.zeros((8, 20))
    with pytest.raises(err, match="dout must be a torch.float16"):
        fn(q.bfloat16(), q, k, k, q, lse, cu)
    with pytest.raises(err, match="dout must be a torch.float16"):
        fn(_t(21, 8, 64), q, k, k, q, lse, cu)
    with pytest.raises(err, match=r"dout must have stride\(-1\) == 1 and stride\(-2\) == head_dim"):
        fn(_t(8, 20, 64).transpose(0, 1), q, k, k, q, lse, cu)   # it is never copied here
    with pytest.raises(err, match="out must be contiguous"):
        fn(q, q, k, k, _t(20, 16, 64)[:, :8], lse, cu)
    with pytest.raises(err, match="lse must be the forward's float32 lse"):
        fn(q, q, k, k, q, lse.double(), cu)
    with pytest.raises(err, match=r"a contiguous \[Hq, T_q\] tensor"):
        fn(q, q, k, k, q, torch.zeros((20, 8)).t(), cu)
    with pytest.raises(err, match="dk must be a contiguous torch.float16 tensor shaped like k"):
        fn(q, q, k, k, q, lse, cu, dk=_t(30, 4, 64)[:, :2])
    with pytest.raises(err, match="q must be a device tensor"):
        fn(_t(20, 16, 64)[:, 8:], q, k, k, q, lse, cu)           # a strided dout passes the checks
    fb = fa_mi355x.flash_attention_bshd_backward
    q4, k4 = _t(3, 10, 8, 64), _t(3, 12, 2, 64)
    good = torch.zeros((8, 30)).view(8, 3, 10).permute(1, 0, 2)
    with pytest.raises(err, match=r"the \[B, Hq, Sq\] view of a \[Hq, B \* Sq\] buffer"):
        fb(q4, q4, k4, k4, q4, torch.zeros((3, 8, 10)))          # a dense [B, Hq, Sq] is another layout
    with pytest.raises(err, match="q must be a device tensor"):
        fb(q4, q4, k4, k4, q4, good)


def test_ops_schemas_fake_and_cpu():
    import fa_mi355x.torch_op  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode

    ops = torch.ops.fa_mi355x
    mid = "Tensor cu_seqlens_q, Tensor? cu_seqlens_k=None, "
    for name, m in (("attn_varlen", mid), ("attn_bshd", "")):
        assert str(getattr(ops, name + "_bwd").default._schema) == (
            "fa_mi355x::%s_bwd(Tensor dout, Tensor q, Tensor k, Tensor v, Tensor out, Tensor lse, %s"
            "bool causal=False) -> (Tensor, Tensor, Tensor)" % (name, m))
        assert str(getattr(ops, name + "_fwd").default._schema) == (
            "fa_mi355x::%s_fwd(Tensor q, Tensor k, Tensor v, %sbool causal=False) -> (Tensor, Tensor)"
            % (name, m))
    q, k, cu = _t(20, 8, 64), _t(30, 2, 64), torch.zeros(4, dtype=torch.int32)
    with pytest.raises(ValueError, match="attn_varlen_bwd needs GPU tensors"):
        ops.attn_varlen_bwd(q, q, k, k, q, torch.zeros((8, 20)), cu)
    with pytest.raises(ValueError, match="attn_bshd_bwd needs GPU tensors"):
        ops.attn_bshd_bwd(q[None], q[None], k[None], k[None], q[None], torch.zeros((1, 8, 20)))
    with pytest.raises(ValueError, match="needs GPU tensors"):
        fa_mi355x.flash_attn_varlen_func(q.requires_grad_(), k, k, cu)
    with pytest.raises(ValueError, match="needs GPU tensors"):
        fa_mi355x.flash_attn_func(q[None], k[None], k[None], causal=True)
    with FakeTensorMode():
        dev = "cuda"
        fq = torch.empty((20, 12, 64), dtype=torch.bfloat16, device=dev)[:, :8]  # a strided view
        fk = torch.empty((30, 2, 64), dtype=torch.bfloat16, device=dev)
        fo = torch.empty((20, 8, 64), dtype=torch.bfloat16, device=dev)
        fl = torch.empty((8, 20), device=dev)
        fcu = torch.empty(4, dtype=torch.int32, device=dev)
        o, l = ops.attn_varlen_fwd(fq, fk, fk, fcu)
        assert o.shape == (20, 8, 64) and o.is_contiguous() and l.shape == (8, 20) and l.dtype is torch.float32
        for g in (ops.attn_varlen_bwd(fo, fq, fk, fk, fo, fl, fcu), ops.attn_varlen_bwd(fo, fq, fk, fk, fo, fl, fcu, fcu, True)):
            assert [tuple(t.shape) for t in g] == [(20, 8, 64), (30, 2, 64), (30, 2, 64)]
            assert all(t.dtype is torch.bfloat16 and t.is_contiguous() for t in g)
        with pytest.raises(Exception, match="expected the forward's float32 lse"):
            ops.attn_varlen_bwd(fo, fq, fk, fk, fo, fl.t(), fcu)
        bq = torch.empty((3, 10, 12, 128), dtype=torch.float16, device=dev)[:, :, :8]
        bk = torch.empty((3, 12, 2, 128), dtype=torch.float16, device=dev)
        bo = torch.empty((3, 10, 8, 128), dtype=torch.float16, device=dev)
        o, l = ops.attn_bshd_fwd(bq, bk, bk, True)
        assert o.shape == (3, 10, 8, 128) and l.shape == (3, 8, 10) and l.stride() == (10, 30, 1)
        g = ops.attn_bshd_bwd(bo, bq, bk, bk, bo, l, True)
        assert [tuple(t.shape) for t in g] == [(3, 10, 8, 128), (3, 12, 2, 128), (3, 12, 2, 128)]
        assert all(t.dtype is torch.float16 and t.is_contiguous() for t in g)
        # the differentiable functions: the forward's shape on the fake GPU tensors ...
        q1 = fq.detach().requires_grad_()
        out = fa_mi355x.flash_attn_varlen_func(q1, fk, fk, fcu, causal=True)
        assert out.shape == (20, 8, 64) and out.dtype is torch.bfloat16 and out.requires_grad
        out = fa_mi355x.flash_attn_func(bq.detach().requires_grad_(), bk, bk)
        assert out.shape == (3, 10, 8, 128) and out.dtype is torch.float16 and out.requires_grad
        # ... and the gradients' shapes on fake CPU tensors (the autograd engine
        # itself needs a device to run a backward on GPU tensors; the ops' fake
        # implementations are the same for both)
        cq = torch.empty((20, 12, 64), dtype=torch.bfloat16)[:, :8].requires_grad_()
        ck, cv = (torch.empty((30, 2, 64), dtype=torch.bfloat16, requires_grad=True) for _ in range(2))
        ccu = torch.empty(4, dtype=torch.int32)
        out = fa_mi355x.flash_attn_varlen_func(cq, ck, cv, ccu, causal=True)
        gq, gk, gv = torch.autograd.grad(out, (cq, ck, cv), torch.empty((8, 20, 64), dtype=torch.bfloat16)
                                         .transpose(0, 1))   # a dout that fails the stride rule
        assert gq.shape == cq.shape and gk.shape == ck.shape and gv.shape == cv.shape
        assert gq.dtype is torch.bfloat16
        q2 = torch.empty((3, 10, 8, 128), dtype=torch.float16, requires_grad=True)
        k2 = torch.empty((3, 12, 2, 128), dtype=torch.float16, requires_grad=True)
        out = fa_mi355x.flash_attn_func(q2, k2, k2)
        gq, gk = torch.autograd.grad(out, (q2, k2), torch.empty_like(out))
        assert gq.shape == q2.shape and gk.shape == k2.shape and gk.dtype is torch.float16
        # the existing ops stay forward-only
        with pytest.raises(RuntimeError, match="forward-only"):
            ops.attn_varlen(q1, fk, fk, fcu)


# ---- the references ------------------------------------------------------------------------------

@pytest.mark.parametrize("causal", [False, True])
def test_reference_against_hand_computed_2x3(causal):
    """2 queries x 3 keys, D = 2, one head, in float64.  Non-causal with these
    numbers row 0's scores are all 0 (q_0 = 0): P_0j = 1/3 exactly.  Causal
    (bottom-right): row 0 sees keys 0 and 1, row 1 all three."""
    q = [[0.0, 0.0], [1.0, -1.0]]
    k = [[1.0, 0.0], [0.0, 2.0], [-1.0, 1.0]]
    v = [[1.0, 2.0], [0.5, -1.0], [3.0, 0.25]]
    do = [[1.0, -2.0], [0.5, 0.25]]
    dq, dk, dv, P = br.formulas_f64(q, k, v, do, causal)
    n0 = 2 if causal else 3
    assert P[0][:n0] == [1.0 / n0] * n0 and P[0][n0:] == [0.0] * (3 - n0)
    e = [math.exp(x / math.sqrt(2)) for x in (1.0, -2.0, -2.0)]   # row 1: q_1 . k_j = 1, -2, -2
    assert P[1] == pytest.approx([x / sum(e) for x in e], rel=1e-15)
    # row 0 (q = 0, uniform P): dV_j gets do_0 / n0 from it, and dK_j gets nothing (q_0 = 0)
    assert dv[2] == pytest.approx([P[1][2] * 0.5 + (0 if causal else 1.0 / 3),
                                   P[1][2] * 0.25 - (0 if causal else 2.0 / 3)], rel=1e-14)
    t = lambda a: torch.tensor(a, dtype=torch.float64)[:, None, :]  # noqa: E731
    cu_q, cu_k = [0, 2], [0, 3]
    got = br.reference(t(q), t(k), t(v), t(do), cu_q, cu_k, causal, False)
    for g, want in zip(got, (dq, dk, dv)):
        assert torch.allclose(g[:, 0], torch.tensor(want, dtype=torch.float64), rtol=1e-12, atol=1e-14)


def test_reference_rows_without_keys_and_gqa():
    """nq > nk under causal: the leading rows see nothing, get dq = 0 and leave
    dk / dv alone; GQA sums the group's heads."""
    g = torch.Generator().manual_seed(1)
    q = torch.randn((5, 4, 8), generator=g, dtype=torch.float64)
    k = torch.randn((3, 2, 8), generator=g, dtype=torch.float64)
    v = torch.randn((3, 2, 8), generator=g, dtype=torch.float64)
    do = torch.randn((5, 4, 8), generator=g, dtype=torch.float64)
    dq, dk, dv = br.reference(q, k, v, do, [0, 5], [0, 3], True, False)
    assert bool((dq[:2] == 0).all()) and bool(torch.isfinite(dq).all())
    for h in range(4):
        lists = [x[:, h].tolist() for x in (q, do)] + [x[:, h // 2].tolist() for x in (k, v)]
        fq, fk, fv, _ = br.formulas_f64(lists[0], lists[2], lists[3], lists[1], True)
        assert torch.allclose(dq[:, h], torch.tensor(fq, dtype=torch.float64), rtol=1e-11, atol=1e-13)
    sums = [[br.formulas_f64(q[:, h].tolist(), k[:, hk].tolist(), v[:, hk].tolist(), do[:, h].tolist(), True)
             for h in (2 * hk, 2 * hk + 1)] for hk in range(2)]
    for hk in range(2):
        want_k = torch.tensor(sums[hk][0][1], dtype=torch.float64) + torch.tensor(sums[hk][1][1], dtype=torch.float64)
        want_v = torch.tensor(sums[hk][0][2], dtype=torch.float64) + torch.tensor(sums[hk][1][2], dtype=torch.float64)
        assert torch.allclose(dk[:, hk], want_k, rtol=1e-11, atol=1e-13)
        assert torch.allclose(dv[:, hk], want_v, rtol=1e-11, atol=1e-13)


@pytest.mark.parametrize("dtype", [br.F16, br.BF16], ids=["fp16", "bf16"])
def test_gate_is_neither_exact_nor_wild(dtype):
    """On the base shape the 16-bit baseline is not exact and not wild: 0 <
    max|g_16 - g_ref| <= 0.05 max|g_ref| per tensor, so the gate neither
    degenerates to one rounding nor admits anything."""
    gref, g16 = br.base_refs(128, dtype, True)
    for name, (base, top, gate) in zip(("dq", "dk", "dv"), br.gate_terms(g16, gref, dtype)):
        print(f"{name}: baseline {base:.3e} max|ref| {top:.3e} gate {gate:.3e}")
        assert 0 < base <= 0.05 * top, (name, base, top)
    # the rows of no sequence are zeros in the references
    for g, own in zip(gref, br.owned_masks()):
        assert bool((g[~own] == 0).all()) and bool(torch.isfinite(g).all())


# ---- the dK/dV kernel's key-block map --------------------------------------------------------

def test_key_block_map_is_the_packed_map_on_cu_seqlens_k():
    """Every key of every sequence lies in exactly one launched block, by the
    packed map on cu_seqlens_k with 128-key blocks; under causal the sweep
    starts at the first 64-row tile holding a row that sees the block's first key."""
    for cu_q, cu_k, tq, tk in ((ar.CU_Q, ar.CU_K, ar.TQ, ar.TK), ([0, 130, 260, 390], [0, 200, 400, 600], 390, 600),
                               ([0, 300, 300], [5, 5, 700], 300, 800)):
        ids = vr.num_ids(tk, len(cu_k) - 1, br.BN)
        for causal in (False, True):
            got = [br.key_block_of(cu_q, cu_k, tq, tk, causal, i) for i in range(ids + 1)]
            assert [None if g is None else g[:2] for g in got] == \
                [vr.block_of(cu_k, tk, br.BN, i) for i in range(ids + 1)]
            assert got[ids] is None
            hits = [g for g in got if g is not None]
            want = {(b, r) for b, (_, n) in enumerate(vr.spans(cu_k, tk)) for r in range(-(-n // br.BN))}
            assert {g[:2] for g in hits} == want and len(hits) == len(want)
            for b, r, j0, nt in hits:
                nq, nk = vr.spans(cu_q, tq)[b][1], vr.spans(cu_k, tk)[b][1]
                vis = br.visible(nq, nk, causal)[:, r * br.BN:(r + 1) * br.BN]
                rows = torch.nonzero(vis.any(1)).flatten().tolist()
                tiles = sorted({t // 64 for t in rows})
                # every tile holding a row that sees a key of the block is swept
                assert all(j0 <= t < j0 + nt for t in tiles), (b, r, j0, nt, tiles[:3])
                # and the sweep starts no earlier than the first row reaching the block's first key
                if causal and rows:
                    first = next(t for t in range(nq) if bool(br.visible(nq, nk, True)[t, r * br.BN]))
                    assert j0 == first // 64
