"""CPU tests of the backward pass through the sliding window and the attention
sinks (fa_attn_bwd_win_* / fa_attn_bwd_sink_*; no GPU): the formulas restated
with plain loops against the autograd reference, an fp32 restatement of what
the kernels compute against the gate, the two loop bounds against brute force,
the four entries' argument statuses, exports and compile-time resource usage,
and the Python wrappers' and torch ops' new arguments.
"""
import ctypes

import pytest
import torch

import attn_bwd_mask_refs as mr
import attn_bwd_refs as br
import attn_varlen_refs as ar
import capi_checks as cc
import fa_mi355x

P = ctypes.c_void_p(0x1000)
INT_MAX = cc.INT_MAX
err = fa_mi355x.FlashAttentionError
OK, NULLP, BAD_D, BAD = (fa_mi355x.FA_OK, fa_mi355x.FA_ERR_NULL_POINTER,
                         fa_mi355x.FA_ERR_UNSUPPORTED_HEAD_DIM, fa_mi355x.FA_ERR_BAD_SHAPE)
F16, BF16 = mr.F16, mr.BF16


# ---- (a) the formulas -----------------------------------------------------------------------------

@pytest.mark.parametrize("causal,window,sink", [(True, 0, 0.3), (True, 2, 0.3), (True, 3, None), (False, 0, -0.7),
                                                (True, 1, 1.5), (True, 2, float("-inf"))])
def test_formulas_against_autograd(causal, window, sink):
    """One head, 5 queries x 7 keys (and 7 x 5: two leading rows see nothing),
    D = 4, float64: plain loops over the contract's formulas, dsinks included,
    against the autograd reference with the sink as an explicit column."""
    for nq, nk in ((5, 7), (7, 5)):
        g = torch.Generator().manual_seed(11)
        q, k, v, do = (torch.randn((n, 1, 4), generator=g, dtype=torch.float64) for n in (nq, nk, nk, nq))
        sinks = None if sink is None else torch.tensor([sink], dtype=torch.float64)
        want = mr.formulas_f64(*(x[:, 0].tolist() for x in (q, k, v, do)), causal, window, sink)
        got = mr.reference(q, k, v, do, [0, nq], [0, nk], causal, False, window, sinks)
        for a, b in zip(got[:3], want[:3]):
            assert torch.allclose(a[:, 0], torch.tensor(b, dtype=torch.float64), rtol=1e-11, atol=1e-13)
        if sink is not None:
            assert float(got[3][0]) == pytest.approx(want[3], rel=1e-11, abs=1e-13)
            if sink == float("-inf"):
                assert float(got[3][0]) == 0.0
        if causal and nq > nk:
            assert bool((got[0][:nq - nk] == 0).all())   # rows that see nothing
        if window > 0 and nk > nq + window - 1:
            assert bool((got[1][:nk - nq - window + 1] == 0).all())   # keys no row sees
            assert bool((got[2][:nk - nq - window + 1] == 0).all())


def test_reference_without_window_and_sinks_is_attn_bwd_refs():
    (qp, kp, vp, dop), cus = br.base_inputs(64, BF16)
    for low in (False, True):
        a = mr.reference(qp, kp, vp, dop, *cus, True, low)
        b = br.reference(qp, kp, vp, dop, *cus, True, low)
        assert all(torch.equal(x, y) for x, y in zip(a, b))
    # a window no shorter than every sequence's keys masks nothing
    a = mr.reference(qp, kp, vp, dop, *cus, True, False, window=max(ar.NK))
    assert all(torch.equal(x, y) for x, y in zip(a, br.reference(qp, kp, vp, dop, *cus, True, False)))


# ---- (b) what the kernels compute, in fp32 ------------------------------------------------------------

@pytest.mark.parametrize("causal,window", [(True, 0), (True, 1), (True, 64), (True, 200), (False, 0)])
@pytest.mark.parametrize("d,dtype", [(128, F16), (64, BF16)], ids=["d128-fp16", "d64-bf16"])
def test_kernel_model_within_three_quarters_of_the_gate(d, dtype, causal, window):
    """out rounded to 16 bits, lse in fp32, P and dS rounded to 16 bits, dsinks
    from the fp32 delta: every tensor within 0.75 of its gate on the base shape
    with sinks, so the gate needs no widening for the window or the sinks."""
    (qp, kp, vp, dop), cus = br.base_inputs(d, dtype)
    sinks = mr.base_sinks()
    got = mr.kernel_model(qp, kp, vp, dop, *cus, causal, window, sinks)
    gref, g16 = mr.base_refs(d, dtype, causal, window, True)
    mr.check_gate(got, gref, g16, dtype, f"model d{d} causal={causal} W={window}", owned=br.owned_masks(), frac=0.75)
    assert float(gref[3].abs().max()) > 0


# ---- (c) the loop bounds -------------------------------------------------------------------------------

@pytest.mark.parametrize("window", [1, 63, 64, 65, 128, 200])
def test_loop_bounds_are_the_brute_force_tiles(window):
    """For every key block (dK/dV) and query block (dQ) of the base shape: the
    swept tiles are exactly the first to the last tile holding a visible (row,
    key) pair; a block without one sweeps at most the one tile its causal
    start names (as before the window), whose elements are all masked."""
    seen_any = 0
    for nq, nk in zip(ar.NQ, ar.NK):
        if nq == 0:
            continue
        vis = mr.visible(nq, nk, True, window)
        for k0 in range(0, nk, br.BN):
            rows = torch.nonzero(vis[:, k0:k0 + br.BN].any(1)).flatten().tolist()
            j0, nt = mr.dkdv_sweep(nq, nk, window, k0)
            if rows:
                assert (j0, j0 + nt - 1) == (rows[0] // mr.BT, rows[-1] // mr.BT), (nq, nk, k0, j0, nt)
                seen_any += 1
            else:
                # no pair: either no tile, or the one tile of the first row past the block's causal edge
                assert nt <= 1, (nq, nk, k0, j0, nt)
        for q0 in range(0, nq, 128):
            keys = torch.nonzero(vis[q0:q0 + 128].any(0)).flatten().tolist()
            jt0, jend = mr.dq_sweep(nq, nk, window, q0)
            if keys:
                assert (jt0, jend - 1) == (keys[0] // mr.BT, keys[-1] // mr.BT), (nq, nk, q0, jt0, jend)
                seen_any += 1
            else:
                assert jend <= jt0 or jend == 0, (nq, nk, q0, jt0, jend)
    assert seen_any >= 10


def test_tile_pairs_is_the_brute_force_count():
    for nq, nk in zip(ar.NQ, ar.NK):
        for window in (0, 1, 64, 200):
            if nq == 0:
                assert mr.tile_pairs(nq, nk, window) == 0
                continue
            vis = mr.visible(nq, nk, True, window)
            want = sum(bool(vis[i:i + 64, j:j + 64].any()) for i in range(0, nq, 64) for j in range(0, nk, 64))
            assert mr.tile_pairs(nq, nk, window) == want, (nq, nk, window)


# ---- (d) exports, resources, statuses --------------------------------------------------------------------

def test_symbols_exported_and_declared():
    cc.assert_exported(mr.SYMBOLS)
    assert not any(s.startswith(("fa_attn_varlen", "fa_decode", "fa_prefill")) for s in mr.SYMBOLS)


def test_no_scratch_and_lds_as_the_twins():
    """Per unit: delta, windowed dK/dV and dQ at two head_dims and the dsinks
    reduction: no scratch (no spills), the LDS of their twins."""
    units = ["fa_attn_bwd_win.hip", "fa_attn_bwd_win_bf16.hip"]
    for unit, rows in zip(units, cc.kernel_resource_usage(units)):
        assert len(rows) == 7, (unit, [r[0] for r in rows])
        for kind, lds_want, n in (("delta", 0, 2), ("dkdv", 2 * 64 * 256 + 512, 2), ("dq", 2 * 64 * 256, 2),
                                  ("dsinks", 4 * 1024 // 64, 1)):
            kernels = [r for r in rows if "fa_attn_bwd_%s_kernel" % kind in r[0]]
            assert len(kernels) == n, (unit, kind)
            for name, scratch, lds in kernels:
                assert scratch == 0 and lds == lds_want, (unit, name, scratch, lds)
                assert kind in ("delta", "dsinks") or "Windowed" in name, name


def _call(fn, variant, dout=P, q=P, k=P, v=P, out=P, lse=P, dq=P, dk=P, dv=P, delta=P, batch=2, hq=8, hkv=2,
          tq=100, tk=120, d=128, cu_q=P, cu_k=P, causal=1, **kw):
    return mr.call(fn, variant, dout, q, k, v, out, lse, dq, dk, dv, delta, batch, hq, hkv, tq, tk, d, cu_q, cu_k,
                   causal, **kw)


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("variant", ["_win", "_sink"])
def test_statuses_in_order(variant, bf16):
    """The window's two statuses in the forward's order, each with every LATER
    check failing too; the rest as for fa_attn_varlen_bwd_*; all returned
    before any HIP call (fake pointers)."""
    fn = mr.entry(fa_mi355x.load_library(), variant, bf16)
    c = lambda **kw: _call(fn, variant, **kw)  # noqa: E731
    # negative counts, then a negative window, then head_dim
    for kw in (dict(batch=-1), dict(hq=-8), dict(hkv=-2), dict(tk=-1), dict(d=-128)):
        assert c(q=None, window=-1, **{"d": 96, **kw}) == BAD, kw
    assert c(window=-1, d=96) == BAD
    assert c(window=0, d=96, tq=-1) == BAD_D
    # total_q, then a window without causal, then the strides
    assert c(tq=-1, window=4, causal=0) == BAD
    assert c(window=4, causal=0, strides=(7, 0, 0, 0), q=None) == BAD
    assert c(window=4, causal=0, batch=0) == BAD       # before the empty-problem returns
    assert c(window=0, causal=0, q=None) == NULLP
    assert c(window=4, causal=1, q=None) == NULLP
    assert c(window=INT_MAX, causal=1, q=None) == NULLP
    assert c(strides=(7, 0, 0, 0), batch=0) == BAD
    # the modes, the empty problems, the heads: as for the entry without a window
    assert c(cu_q=None, cu_k=P, batch=0) == BAD
    assert c(cu_q=None, cu_k=None, seqlen=(50, 61), q=None) == BAD
    assert c(cu_q=None, cu_k=None, seqlen=(50, 60), q=None, window=3) == NULLP
    nothing = dict(dout=None, q=None, k=None, v=None, out=None, lse=None, dq=None, delta=None)
    assert c(hq=0, hkv=3, **nothing, dk=None, dv=None) == OK
    for kw in (dict(batch=0), dict(tq=0)):
        assert c(**nothing, dk=None, hkv=3, **kw) == NULLP, kw
        assert c(**nothing, dk=None, dv=None, hkv=3, tk=0, **kw) == OK, kw
    for hq, hkv in ((8, 3), (7, 2), (4, 8), (8, 0)):
        assert c(hq=hq, hkv=hkv, q=None) == BAD
    assert c(tq=INT_MAX // 8 + 1, q=None) == BAD
    assert c(tk=INT_MAX - 63, q=None) == BAD
    # the windowed kernels' own range: total_q + total_k in an int
    assert c(hq=1, hkv=1, tq=INT_MAX // 2 + 1, tk=INT_MAX // 2 + 1, q=None) == BAD
    assert c(hq=1, hkv=1, tq=INT_MAX // 2, tk=INT_MAX // 2, q=None) == NULLP
    assert c(tk=0, dq=None) == NULLP
    for bad in ("dout", "q", "k", "v", "out", "lse", "dq", "dk", "dv", "delta"):
        assert c(**{bad: None}) == NULLP, bad
    if variant == "_sink":
        # sinks without dsinks: the last NULL pointer; without sinks dsinks may be absent (no launch is
        # reached here: a NULL pointer before it answers)
        assert c(sinks=P, dsinks=None) == NULLP
        assert c(sinks=P, dsinks=None, window=-1) == BAD


# ---- the Python wrappers and the torch ops -------------------------------------------------------------

def _t(*shape, dtype=torch.float16):
    return torch.zeros(shape, dtype=dtype)


def test_wrapper_refusals():
    """Refused before the device is looked at, so CPU tensors reach every message."""
    fn = fa_mi355x.flash_attention_varlen_backward
    q, k, cu = _t(20, 8, 64), _t(30, 2, 64), torch.zeros(4, dtype=torch.int32)
    lse = torch.zeros((8, 20))
    with pytest.raises(err, match="window must be >= 0"):
        fn(q, q, k, k, q, lse, cu, causal=True, window=-1)
    with pytest.raises(err, match="a window needs causal=True"):
        fn(q, q, k, k, q, lse, cu, window=4)
    with pytest.raises(err, match="window must be an int"):
        fn(q, q, k, k, q, lse, cu, causal=True, window=4.0)
    with pytest.raises(err, match=r"sinks must be a contiguous float32 \[Hq = 8\] tensor"):
        fn(q, q, k, k, q, lse, cu, sinks=torch.zeros(7))
    with pytest.raises(err, match=r"sinks must be a contiguous float32 \[Hq = 8\] tensor"):
        fn(q, q, k, k, q, lse, cu, sinks=torch.zeros(8, dtype=torch.float64))
    with pytest.raises(err, match="dsinks is the gradient of sinks"):
        fn(q, q, k, k, q, lse, cu, dsinks=torch.zeros(8))
    with pytest.raises(err, match=r"dsinks must be a contiguous float32 \[Hq = 8\] tensor"):
        fn(q, q, k, k, q, lse, cu, sinks=torch.zeros(8), dsinks=torch.zeros(16)[::2])
    with pytest.raises(err, match="q must be a device tensor"):
        fn(q, q, k, k, q, lse, cu, causal=True, window=4, sinks=torch.zeros(8), dsinks=torch.zeros(8))
    fb = fa_mi355x.flash_attention_bshd_backward
    q4, k4 = _t(3, 10, 8, 64), _t(3, 12, 2, 64)
    good = torch.zeros((8, 30)).view(8, 3, 10).permute(1, 0, 2)
    with pytest.raises(err, match="a window needs causal=True"):
        fb(q4, q4, k4, k4, q4, good, window=1)
    with pytest.raises(err, match="q must be a device tensor"):
        fb(q4, q4, k4, k4, q4, good, causal=True, window=1, sinks=torch.zeros(8))


def test_ops_schemas_fake_and_cpu():
    import fa_mi355x.torch_op  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode

    ops = torch.ops.fa_mi355x
    mid = "Tensor cu_seqlens_q, Tensor? cu_seqlens_k=None, "
    for name, m in (("attn_varlen", mid), ("attn_bshd", "")):
        for ov, tail, ret in (("window", ", int window=0", ""), ("sinks", ", int window=0, Tensor? sinks=None", ", Tensor")):
            assert str(getattr(getattr(ops, name + "_bwd"), ov)._schema) == (
                "fa_mi355x::%s_bwd.%s(Tensor dout, Tensor q, Tensor k, Tensor v, Tensor out, Tensor lse, %s"
                "bool causal=False%s) -> (Tensor, Tensor, Tensor%s)" % (name, ov, m, tail, ret))
            assert str(getattr(getattr(ops, name + "_fwd"), ov)._schema) == (
                "fa_mi355x::%s_fwd.%s(Tensor q, Tensor k, Tensor v, %sbool causal=False%s) -> (Tensor, Tensor)"
                % (name, ov, m, tail))
        # the base schemas stand as they were
        assert str(getattr(ops, name + "_bwd").default._schema).endswith("bool causal=False) -> (Tensor, Tensor, Tensor)")
    q, k, cu = _t(20, 8, 64), _t(30, 2, 64), torch.zeros(4, dtype=torch.int32)
    sk = torch.zeros(8)
    with pytest.raises(ValueError, match="attn_varlen_bwd needs GPU tensors"):
        ops.attn_varlen_bwd(q, q, k, k, q, torch.zeros((8, 20)), cu, None, True, 4)
    with pytest.raises(ValueError, match="attn_bshd_bwd needs GPU tensors"):
        ops.attn_bshd_bwd(q[None], q[None], k[None], k[None], q[None], torch.zeros((1, 8, 20)), True, 4, sk)
    with pytest.raises(ValueError, match="needs GPU tensors"):
        fa_mi355x.flash_attn_varlen_func(q.requires_grad_(), k, k, cu, causal=True, window=4, sinks=sk)
    with pytest.raises(ValueError, match="needs GPU tensors"):
        fa_mi355x.flash_attn_func(q[None], k[None], k[None], causal=True, window=4)
    with FakeTensorMode():
        dev = "cuda"
        fq = torch.empty((20, 12, 64), dtype=torch.bfloat16, device=dev)[:, :8]
        fk = torch.empty((30, 2, 64), dtype=torch.bfloat16, device=dev)
        fo = torch.empty((20, 8, 64), dtype=torch.bfloat16, device=dev)
        fl = torch.empty((8, 20), device=dev)
        fcu = torch.empty(4, dtype=torch.int32, device=dev)
        fs = torch.empty(8, device=dev)
        for extra in ((True, 4), (True, 4, fs), (False, 0, fs)):
            o, l = ops.attn_varlen_fwd(fq, fk, fk, fcu, None, *extra)
            assert o.shape == (20, 8, 64) and o.is_contiguous() and l.shape == (8, 20) and l.dtype is torch.float32
            g = ops.attn_varlen_bwd(fo, fq, fk, fk, fo, fl, fcu, None, *extra)
            assert [tuple(t.shape) for t in g[:3]] == [(20, 8, 64), (30, 2, 64), (30, 2, 64)]
            assert all(t.dtype is torch.bfloat16 and t.is_contiguous() for t in g[:3])
            assert len(g) == len(extra) + 1
            if len(g) == 4:
                assert g[3].shape == (8,) and g[3].dtype is torch.float32
        # the packet resolves by the arguments given: the base overload still answers its own calls
        assert len(ops.attn_varlen_bwd(fo, fq, fk, fk, fo, fl, fcu, None, True)) == 3
        with pytest.raises(Exception, match="expected window >= 0"):
            ops.attn_varlen_bwd(fo, fq, fk, fk, fo, fl, fcu, None, True, -1)
        with pytest.raises(Exception, match=r"expected a float32 \[Hq\] sinks"):
            ops.attn_varlen_fwd(fq, fk, fk, fcu, None, True, 0, fs.double())
        bq = torch.empty((3, 10, 12, 128), dtype=torch.float16, device=dev)[:, :, :8]
        bk = torch.empty((3, 12, 2, 128), dtype=torch.float16, device=dev)
        bo = torch.empty((3, 10, 8, 128), dtype=torch.float16, device=dev)
        o, l = ops.attn_bshd_fwd(bq, bk, bk, True, 4, fs)
        assert o.shape == (3, 10, 8, 128) and l.shape == (3, 8, 10) and l.stride() == (10, 30, 1)
        g = ops.attn_bshd_bwd(bo, bq, bk, bk, bo, l, True, 4, fs)
        assert [tuple(t.shape) for t in g] == [(3, 10, 8, 128), (3, 12, 2, 128), (3, 12, 2, 128), (8,)]
        assert len(ops.attn_bshd_bwd(bo, bq, bk, bk, bo, l, True, 4)) == 3
        # the differentiable functions: the forward's shape on the fake GPU tensors ...
        out = fa_mi355x.flash_attn_varlen_func(fq.detach().requires_grad_(), fk, fk, fcu, causal=True, window=4,
                                               sinks=fs.detach().requires_grad_())
        assert out.shape == (20, 8, 64) and out.dtype is torch.bfloat16 and out.requires_grad
        # ... and the gradients' shapes, the sinks' among them, on fake CPU tensors
        cq = torch.empty((20, 12, 64), dtype=torch.bfloat16)[:, :8].requires_grad_()
        ck, cv = (torch.empty((30, 2, 64), dtype=torch.bfloat16, requires_grad=True) for _ in range(2))
        cs = torch.empty(8, requires_grad=True)
        ccu = torch.empty(4, dtype=torch.int32)
        out = fa_mi355x.flash_attn_varlen_func(cq, ck, cv, ccu, causal=True, window=4, sinks=cs)
        gq, gk, gv, gs = torch.autograd.grad(out, (cq, ck, cv, cs), torch.empty((20, 8, 64), dtype=torch.bfloat16))
        assert gq.shape == cq.shape and gk.shape == ck.shape and gv.shape == cv.shape
        assert gs.shape == (8,) and gs.dtype is torch.float32
        out = fa_mi355x.flash_attn_varlen_func(cq, ck, cv, ccu, causal=True, window=4)
        gq, gk = torch.autograd.grad(out, (cq, ck), torch.empty((20, 8, 64), dtype=torch.bfloat16))
        assert gq.shape == cq.shape and gk.shape == ck.shape
        q2 = torch.empty((3, 10, 8, 128), dtype=torch.float16, requires_grad=True)
        k2 = torch.empty((3, 12, 2, 128), dtype=torch.float16, requires_grad=True)
        out = fa_mi355x.flash_attn_func(q2, k2, k2, causal=True, sinks=cs)
        gq, gk, gs = torch.autograd.grad(out, (q2, k2, cs), torch.empty_like(out))
        assert gq.shape == q2.shape and gk.shape == k2.shape and gs.shape == (8,)
