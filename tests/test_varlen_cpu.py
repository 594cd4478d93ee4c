"""CPU tests of the packed (cu_seqlens) prefill and cache-append entries (no
GPU): the workgroup map of csrc/fa_varlen_map.hpp as a property over random
cu_seqlens, pack / unpack of tests/varlen_refs.py, the fourteen symbols and
their argument statuses (all returned before any launch, so fake pointers
suffice), the Python wrappers' rejections on CPU tensors, the torch ops'
schemas, and the compile-time resource usage of the five new units.
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import capi_checks as cc
import decode_refs as dr
import fa_mi355x
import prefill_refs as pr
import varlen_refs as vr

FP8 = torch.float8_e4m3fn
INT_MAX = cc.INT_MAX
P = ctypes.c_void_p(0x1000)
err = fa_mi355x.FlashAttentionError

PRE_ENTRIES = [(paged, kv8, bf16) for paged in (False, True) for kv8 in (False, True) for bf16 in (False, True)]
PRE_SYMBOLS = ["fa_prefill_varlen" + ("_paged" if p else "") + ("_kv8" if k else "") + ("_bf16" if b else "_f16")
               for p, k, b in PRE_ENTRIES]
APP_ENTRIES = [(False, False, None), (True, False, None), (False, True, False), (False, True, True),
               (True, True, False), (True, True, True)]
APP_SYMBOLS = ["fa_cache_append_varlen" + ("_paged" if p else "")
               + (("_kv8_bf16" if b else "_kv8_f16") if k else "_16") for p, k, b in APP_ENTRIES]


def test_symbols_exported_and_declared():
    assert len(set(PRE_SYMBOLS + APP_SYMBOLS)) == 14
    cc.assert_exported(PRE_SYMBOLS + APP_SYMBOLS)


# ---- the workgroup map ---------------------------------------------------------------

def _random_cu(rng, bt):
    """Token counts with empty sequences, starts on and off multiples of bt, and
    (every other draw) a total that is a multiple of bt; now and then cu[0] > 0
    and a tail of unowned rows."""
    nseq = int(rng.integers(1, 12))
    n = [int(rng.choice([0, 0, 1, bt - 1, bt, bt + 1, 2 * bt, int(rng.integers(0, 3 * bt + 2))]))
         for _ in range(nseq)]
    start = int(rng.choice([0, 0, 1, bt, int(rng.integers(0, 2 * bt))]))
    tail = int(rng.choice([0, 0, 1, bt, int(rng.integers(0, bt))]))
    total = start + sum(n) + tail
    if rng.integers(0, 2) and total % bt:
        total += bt - total % bt
    return vr.cu_of(n, start), n, total


@pytest.mark.parametrize("bt", [128, 64])
def test_map_hits_every_block_exactly_once(bt):
    """Every (b, r) with bt * r < n_b is the answer of exactly one virtual block
    id below T / bt + B (what the host launches from shapes alone), and every
    other id answers "return".  bt = 128: prefill's query blocks and append's
    blocks at head_dim 64; bt = 64: append's at head_dim 128."""
    rng = np.random.default_rng(bt)
    saw_empty = saw_aligned = saw_unaligned = saw_mult = False
    for _ in range(400):
        cu, n, total = _random_cu(rng, bt)
        nseq = len(n)
        f = vr.f_map(cu, total, bt)
        assert all(a < b for a, b in zip(f, f[1:])), (cu, f)      # strictly increasing
        assert f[-1] <= vr.num_ids(total, nseq, bt), (cu, total)   # the launch covers every range
        want = {(b, r) for b, nb in enumerate(n) for r in range(-(-nb // bt))}
        got = [vr.block_of(cu, total, bt, i) for i in range(vr.num_ids(total, nseq, bt))]
        hits = [x for x in got if x is not None]
        assert len(hits) == len(set(hits)), (cu, total, hits)
        assert set(hits) == want, (cu, total)
        for b, nb in enumerate(n):
            assert f[b + 1] - f[b] >= -(-nb // bt), (cu, b)
        # ids past the launch answer "return" too (f(B) bounds them)
        assert vr.block_of(cu, total, bt, vr.num_ids(total, nseq, bt)) is None
        saw_empty |= 0 in n
        saw_aligned |= any(c % bt == 0 and nb for c, nb in zip(cu, n))
        saw_unaligned |= any(c % bt and nb for c, nb in zip(cu, n))
        saw_mult |= total % bt == 0
    assert saw_empty and saw_aligned and saw_unaligned and saw_mult


@pytest.mark.parametrize("bt", [128, 64])
def test_map_is_in_bounds_for_any_cu(bt):
    """Garbage cu (negative, past T, decreasing): whatever the map answers, the
    rows it names lie inside [0, T)."""
    rng = np.random.default_rng(7 + bt)
    for _ in range(300):
        nseq = int(rng.integers(1, 9))
        total = int(rng.integers(1, 5 * bt))
        cu = [int(x) for x in rng.integers(-2 * bt, total + 2 * bt, nseq + 1)]
        if rng.integers(0, 4) == 0:
            cu[int(rng.integers(0, nseq + 1))] = int(rng.choice([-2 ** 31, 2 ** 31 - 1]))
        sp = vr.spans(cu, total)
        for i in range(vr.num_ids(total, nseq, bt)):
            hit = vr.block_of(cu, total, bt, i)
            if hit is None:
                continue
            b, r = hit
            s, n = sp[b]
            assert 0 <= b < nseq and r >= 0 and bt * r < n, (cu, total, i, hit)
            assert 0 <= s and s + n <= total, (cu, total, i, hit)


def test_base_shape_of_the_gpu_tests():
    """n = (0, 1, 127, 128, 321): starts 0, 0, 1, 128, 256; T = 600 leaves a tail."""
    n = (0, 1, 127, 128, 321)
    cu = vr.cu_of(n)
    assert cu == [0, 0, 1, 128, 256, 577]
    assert vr.spans(cu, 600) == [(0, 0), (0, 1), (1, 127), (128, 128), (256, 321)]
    assert vr.f_map(cu, 600, 128) == [0, 1, 2, 4, 6, 9]
    got = [vr.block_of(cu, 600, 128, i) for i in range(vr.num_ids(600, 5, 128))]
    assert got == [None, (1, 0), (2, 0), None, (3, 0), None, (4, 0), (4, 1), (4, 2)]
    assert int(vr.owned_rows(cu, 600).sum()) == 577


# ---- pack / unpack -------------------------------------------------------------------

def test_pack_unpack_round_trip_and_contract():
    """unpack(pack(x)) returns the rows t < n_b; the float64 contract on the
    unpacked tensors (what the GPU tests hold the packed entries to) is the
    contract on the padded originals."""
    b, hq, hkv, smax, cap, d = 3, 4, 2, 40, 96, 64
    n, kv_lens = (40, 0, 23), (70, 5, 23)
    q, k, v = dr.inputs(b, hq, hkv, smax, cap, d)
    cu = vr.cu_of(n, start=3)
    qp = vr.pack(q, n, total=70, start=3, fill=0x7e00)
    assert qp.shape == (70, hq, d)
    own = vr.owned_rows(cu, 70)
    assert int(own.sum()) == sum(n) and (qp[~own] == 0x7e00).all()
    back = vr.unpack(qp, cu, smax)
    for bi, nb in enumerate(n):
        assert np.array_equal(back[bi, :, :nb], q[bi, :, :nb])
        assert not back[bi, :, nb:].any()
    tq = torch.from_numpy(np.array(q).view(np.int16)).view(torch.float16)
    tp = vr.pack(tq, n, total=70, start=3)
    assert torch.equal(vr.unpack(tp, cu, smax)[0], tq[0])
    lse = torch.arange(4 * 70, dtype=torch.float32).reshape(4, 70)
    ul = vr.unpack(lse, cu, smax, fill=float("-inf"))
    assert ul.shape == (3, 4, 40) and torch.equal(ul[2, :, :23], lse[:, 43:66])
    f64 = [a.view(np.float16).astype(np.float64) for a in (q, k, v)]
    want = pr.contract_f64(*f64, kv_lens, n, True)
    got = pr.contract_f64(back.view(np.float16).astype(np.float64), f64[1], f64[2], kv_lens, n, True)
    for w, g in zip(want, got):
        assert np.array_equal(w, g, equal_nan=True)


# ---- the C entries' argument statuses ------------------------------------------------

def _pre(entry, q, k, v, o, b, hq, hkv, total, cap, d, lens=None, cu=P, causal=1, table=P, npages=100,
         psz=128, mpp=None):
    paged, kv8, _ = entry
    fn = getattr(fa_mi355x.load_library(), PRE_SYMBOLS[PRE_ENTRIES.index(entry)])
    tail = (None, None) if kv8 else ()
    if paged:
        pages = cap // psz if mpp is None and psz > 0 else (mpp or 0)
        return fn(q, k, v, o, None, b, hq, hkv, total, d, npages, psz, table, pages, lens, cu, causal, None,
                  *tail)
    return fn(q, k, v, o, None, b, hq, hkv, total, cap, d, lens, cu, causal, None, *tail)


@pytest.mark.parametrize("entry", PRE_ENTRIES, ids=PRE_SYMBOLS)
def test_prefill_varlen_argument_statuses(entry):
    """The status table of include/fa_mi355x.h, in fa_prefill_*'s order.  Every
    call returns before any launch: an argument error, an empty problem, or --
    where a shape must be shown to be ACCEPTED -- the NULL q that is looked at
    after every shape."""
    fa = fa_mi355x
    paged = entry[0]
    call = lambda *a, **kw: _pre(entry, *a, **kw)  # noqa: E731
    for bad in range(4):  # each of q, k, v, o NULL in turn
        ptrs = [None if i == bad else P for i in range(4)]
        assert call(*ptrs, 3, 8, 2, 300, 1024, 128) == fa.FA_ERR_NULL_POINTER
    # cu_seqlens_q is required
    assert call(P, P, P, P, 3, 8, 2, 300, 1024, 128, cu=None) == fa.FA_ERR_NULL_POINTER
    for d in (0, 32, 96, 256):
        assert call(P, P, P, P, 3, 8, 2, 300, 1024, d) == fa.FA_ERR_UNSUPPORTED_HEAD_DIM
    for hq, hkv in ((8, 3), (7, 2), (4, 8)):
        assert call(P, P, P, P, 3, hq, hkv, 300, 1024, 128) == fa.FA_ERR_BAD_SHAPE
    assert call(P, P, P, P, 3, 8, 2, -1, 1024, 128) == fa.FA_ERR_BAD_SHAPE
    assert call(P, P, P, P, -1, 8, 2, 300, 1024, 128) == fa.FA_ERR_BAD_SHAPE
    assert call(P, P, P, P, 3, -8, 2, 300, 1024, 128) == fa.FA_ERR_BAD_SHAPE
    assert call(P, P, P, P, 3, 8, -2, 300, 1024, 128) == fa.FA_ERR_BAD_SHAPE
    # accepted as shapes: any total, more sequences than tokens
    for total, b in ((1, 1), (17, 40), (4096, 1), (1 << 20, 64)):
        assert call(None, P, P, P, b, 8, 2, total, 1024, 128) == fa.FA_ERR_NULL_POINTER, (total, b)
    # the 32-bit limits: heads_q * total_q LSE rows ...
    assert call(P, P, P, P, 1, 64, 64, 1 << 25, 1024, 128) == fa.FA_ERR_BAD_SHAPE
    assert call(None, P, P, P, 1, 64, 64, (1 << 25) - 1, 1024, 128) == fa.FA_ERR_NULL_POINTER
    # ... 128 * heads_q * 2 * head_dim bytes of one block's rows ...
    assert call(P, P, P, P, 1, 1 << 16, 1, 128, 1024, 128) == fa.FA_ERR_BAD_SHAPE
    assert call(P, P, P, P, 1, 1 << 17, 1, 128, 1024, 64) == fa.FA_ERR_BAD_SHAPE
    assert call(None, P, P, P, 1, (1 << 16) - 1, 1, 128, 1024, 128) == fa.FA_ERR_NULL_POINTER
    # ... and heads_q * (total_q / 128 + batch) workgroups
    assert call(P, P, P, P, 1 << 27, 16, 16, 128, 1024, 128) == fa.FA_ERR_BAD_SHAPE
    assert call(None, P, P, P, (1 << 27) - 2, 16, 16, 128, 1024, 128) == fa.FA_ERR_NULL_POINTER
    assert call(P, P, P, P, INT_MAX, 1, 1, 128, 1024, 128) == fa.FA_ERR_BAD_SHAPE
    if paged:
        assert call(P, P, P, P, 3, 8, 2, 300, 1024, 128, table=None) == fa.FA_ERR_NULL_POINTER
        for psz in (0, 32, 96, -64, 1, 63, 65):
            assert call(P, P, P, P, 3, 8, 2, 300, 1024, 128, psz=psz, mpp=8) == fa.FA_ERR_BAD_SHAPE, psz
        for npages in (0, -1):
            assert call(P, P, P, P, 3, 8, 2, 300, 1024, 128, npages=npages) == fa.FA_ERR_BAD_SHAPE
        assert call(P, P, P, P, 3, 8, 2, 300, 1024, 128, mpp=-1) == fa.FA_ERR_BAD_SHAPE
        assert call(P, P, P, P, 3, 8, 2, 300, 0, 128, psz=64, mpp=2147483520 // 64 + 1) == fa.FA_ERR_BAD_SHAPE
        assert call(None, P, P, P, 3, 8, 2, 300, 0, 128, psz=64, mpp=2147483520 // 64) == \
            fa.FA_ERR_NULL_POINTER
        assert call(P, P, P, P, 3, 8, 2, 300, 0, 128, npages=1, psz=1 << 23, mpp=1) == fa.FA_ERR_BAD_SHAPE
    else:
        assert call(P, P, P, P, 3, 8, 2, 300, -5, 128) == fa.FA_ERR_BAD_SHAPE
        assert call(P, P, P, P, 3, 8, 2, 300, 8388608, 128) == fa.FA_ERR_BAD_SHAPE
        assert call(P, P, P, P, 3, 8, 2, 300, 16777216, 64) == fa.FA_ERR_BAD_SHAPE
        assert call(None, P, P, P, 3, 8, 2, 300, 8388607, 128) == fa.FA_ERR_NULL_POINTER
    # empty problems: nothing to do, nothing launched, no pointer looked at
    assert call(None, None, None, None, 0, 8, 2, 300, 1024, 128, table=None, cu=None) == fa.FA_OK
    assert call(None, None, None, None, 3, 0, 0, 300, 1024, 128, table=None, cu=None) == fa.FA_OK
    assert call(None, None, None, None, 3, 8, 2, 0, 1024, 128, table=None, cu=None) == fa.FA_OK
    if paged:  # ... but the page geometry is still checked
        assert call(None, None, None, None, 3, 8, 2, 0, 1024, 128, table=None, psz=96, mpp=8) == \
            fa.FA_ERR_BAD_SHAPE
    # rows but no keys: only o is needed (and missing here)
    assert call(None, None, None, None, 3, 8, 2, 300, 0, 128, table=None, mpp=0, cu=None) == \
        fa.FA_ERR_NULL_POINTER


def _app(entry, kn, vn, kc, vc, b, hkv, total, cap, d, lens=P, cu=P, table=P, npages=100, psz=128,
         mpp=None):
    paged, kv8, _ = entry
    fn = getattr(fa_mi355x.load_library(), APP_SYMBOLS[APP_ENTRIES.index(entry)])
    tail = (None, None) if kv8 else ()
    if paged:
        pages = cap // psz if mpp is None and psz > 0 else (mpp or 0)
        return fn(kn, vn, kc, vc, b, hkv, total, d, npages, psz, table, pages, lens, cu, None, *tail)
    return fn(kn, vn, kc, vc, b, hkv, total, cap, d, lens, cu, None, *tail)


@pytest.mark.parametrize("entry", APP_ENTRIES, ids=APP_SYMBOLS)
def test_append_varlen_argument_statuses(entry):
    """fa_cache_append_*'s table with total_new and a required cu_seqlens."""
    fa = fa_mi355x
    paged = entry[0]
    call = lambda *a, **kw: _app(entry, *a, **kw)  # noqa: E731
    for bad in range(4):  # each of k_new, v_new and the caches NULL in turn
        ptrs = [None if i == bad else P for i in range(4)]
        assert call(*ptrs, 3, 2, 300, 1024, 128) == fa.FA_ERR_NULL_POINTER
    assert call(P, P, P, P, 3, 2, 300, 1024, 128, cu=None) == fa.FA_ERR_NULL_POINTER
    assert call(P, P, P, P, 3, 2, 300, 1024, 128, lens=None) == fa.FA_ERR_NULL_POINTER
    for d in (0, 32, 96, 256):
        assert call(P, P, P, P, 3, 2, 300, 1024, d) == fa.FA_ERR_UNSUPPORTED_HEAD_DIM
    assert call(P, P, P, P, -1, 2, 300, 1024, 128) == fa.FA_ERR_BAD_SHAPE
    assert call(P, P, P, P, 3, -2, 300, 1024, 128) == fa.FA_ERR_BAD_SHAPE
    assert call(P, P, P, P, 3, 2, -1, 1024, 128) == fa.FA_ERR_BAD_SHAPE
    assert call(P, P, P, P, 3, 2, INT_MAX - 63, 1024, 128) == fa.FA_ERR_BAD_SHAPE
    assert call(None, P, P, P, 3, 2, INT_MAX - 64, 1024, 128) == fa.FA_ERR_NULL_POINTER
    # total_new / TB + batch virtual blocks past INT_MAX (TB 64 at head_dim 128, 128 at 64)
    assert call(P, P, P, P, INT_MAX, 2, 64, 1024, 128) == fa.FA_ERR_BAD_SHAPE
    assert call(None, P, P, P, INT_MAX - 1, 2, 64, 1024, 128) == fa.FA_ERR_NULL_POINTER
    assert call(None, P, P, P, INT_MAX, 2, 64, 1024, 64) == fa.FA_ERR_NULL_POINTER
    assert call(P, P, P, P, INT_MAX, 2, 128, 1024, 64) == fa.FA_ERR_BAD_SHAPE
    if paged:
        assert call(P, P, P, P, 3, 2, 300, 1024, 128, table=None) == fa.FA_ERR_NULL_POINTER
        for psz in (0, 32, 96, -64, 1, 63, 65):
            assert call(P, P, P, P, 3, 2, 300, 1024, 128, psz=psz, mpp=8) == fa.FA_ERR_BAD_SHAPE, psz
        for npages in (0, -1):
            assert call(P, P, P, P, 3, 2, 300, 1024, 128, npages=npages) == fa.FA_ERR_BAD_SHAPE
        assert call(P, P, P, P, 3, 2, 300, 1024, 128, mpp=-1) == fa.FA_ERR_BAD_SHAPE
        assert call(P, P, P, P, 3, 2, 300, 0, 128, psz=64, mpp=2147483520 // 64 + 1) == fa.FA_ERR_BAD_SHAPE
        assert call(P, P, P, P, 3, 2, 300, 0, 128, npages=1, psz=1 << 23, mpp=1) == fa.FA_ERR_BAD_SHAPE
    else:
        assert call(P, P, P, P, 3, 2, 300, -5, 128) == fa.FA_ERR_BAD_SHAPE
        assert call(P, P, P, P, 3, 2, 300, 8388608, 128) == fa.FA_ERR_BAD_SHAPE
        assert call(None, P, P, P, 3, 2, 300, 8388607, 128) == fa.FA_ERR_NULL_POINTER
    # nothing to do: no sequence, no head, no token, no cache row
    for b, hkv, total, cap in ((0, 2, 300, 1024), (3, 0, 300, 1024), (3, 2, 0, 1024), (3, 2, 300, 0)):
        assert call(None, None, None, None, b, hkv, total, cap, 128, lens=None, cu=None, table=None,
                    mpp=None if cap else 0) == fa.FA_OK, (b, hkv, total, cap)
    if paged:
        assert call(None, None, None, None, 3, 2, 0, 1024, 128, psz=96, mpp=8) == fa.FA_ERR_BAD_SHAPE


# ---- the Python wrappers on CPU tensors: every rejection names its own cause ---------

def _t(shape, dtype=torch.float16):
    return torch.zeros(shape, dtype=torch.float32).to(dtype)


def _i32(*v):
    return torch.tensor(v, dtype=torch.int32)


def test_prefill_varlen_wrapper_rejections():
    f = fa_mi355x.flash_attention_prefill_varlen
    q, k, cu = _t((30, 4, 64)), _t((2, 2, 128, 64)), _i32(0, 10, 30)
    with pytest.raises(err, match="q must be float16 or bfloat16"):
        f(q.float(), k, k, cu)
    with pytest.raises(err, match="k_cache and v_cache must have one dtype"):
        f(q, k.to(FP8), k, cu)
    with pytest.raises(err, match=r"q must be 3-D \[T,H,D\]"):
        f(q[None], k, k, cu)
    with pytest.raises(err, match=r"k_cache must be 4-D \(BHSD\)"):
        f(q, k[0], k, cu)
    with pytest.raises(err, match=r"q must be contiguous \[T,H,D\]"):
        f(q.transpose(0, 1), k, k, cu)
    with pytest.raises(err, match=r"out must be \[T,H,D\] like q"):
        f(q, k, k, cu, out=_t((31, 4, 64)))
    with pytest.raises(err, match="q and the caches must agree in head_dim"):
        f(q, _t((2, 2, 128, 128)), _t((2, 2, 128, 128)), cu)
    with pytest.raises(err, match="cu_seqlens_q is required") as e:
        f(q, k, k, None)
    assert e.value.status == fa_mi355x.FA_ERR_NULL_POINTER
    with pytest.raises(err, match="cu_seqlens_q must be int32, got torch.int64"):
        f(q, k, k, torch.tensor([0, 10, 30]))
    with pytest.raises(err, match=r"cu_seqlens_q must be a contiguous \[B \+ 1 = 3\] tensor, got \[2\]"):
        f(q, k, k, _i32(0, 30))
    with pytest.raises(err, match=r"cu_seqlens_q must be a contiguous \[B \+ 1 = 3\] tensor"):
        f(q, k, k, _i32(0, 1, 2, 3, 4, 5)[::2])
    with pytest.raises(err, match="heads_q 4 is not a multiple of heads_kv 3"):
        f(q, _t((2, 3, 128, 64)), _t((2, 3, 128, 64)), cu)
    with pytest.raises(err, match=r"kv_lens must be a contiguous \[B\] tensor"):
        f(q, k, k, cu, kv_lens=_i32(1, 2, 3))
    with pytest.raises(err, match="go with a torch.float8_e4m3fn cache only"):
        f(q, k, k, cu, k_scale=torch.ones(2))
    # all shapes and dtypes in order: what is left is where the tensors live
    with pytest.raises(err, match="q must be a device tensor") as e:
        f(q, k, k, cu, kv_lens=_i32(50, 60))
    assert e.value.status == fa_mi355x.FA_ERR_NULL_POINTER


def test_prefill_varlen_paged_wrapper_rejections():
    f = fa_mi355x.flash_attention_prefill_varlen_paged
    q, pool = _t((30, 4, 64), torch.bfloat16), _t((5, 2, 128, 64), torch.bfloat16)
    table, cu = torch.zeros((2, 3), dtype=torch.int32), _i32(0, 10, 30)
    with pytest.raises(err, match="block_table is required"):
        f(q, pool, pool, None, cu)
    with pytest.raises(err, match="page_size 96 is not a positive multiple of 64"):
        f(q, _t((5, 2, 96, 64), torch.bfloat16), _t((5, 2, 96, 64), torch.bfloat16), table, cu)
    with pytest.raises(err, match="block_table must be int32"):
        f(q, pool, pool, table.long(), cu)
    with pytest.raises(err, match="block_table must be 2-D"):
        f(q, pool, pool, table[0], cu)
    # B is the table's row count
    with pytest.raises(err, match=r"cu_seqlens_q must be a contiguous \[B \+ 1 = 4\] tensor"):
        f(q, pool, pool, torch.zeros((3, 3), dtype=torch.int32), cu)
    with pytest.raises(err, match="q must be a device tensor"):
        f(q, pool, pool, table, cu)


def test_append_varlen_wrapper_rejections():
    f = fa_mi355x.flash_attention_cache_append_varlen
    fp = fa_mi355x.flash_attention_cache_append_varlen_paged
    kn, k, cu, lens = _t((30, 2, 64)), _t((2, 2, 128, 64)), _i32(0, 10, 30), _i32(10, 20)
    with pytest.raises(err, match="k_new must be float16 or bfloat16"):
        f(kn.float(), kn.float(), k, k, cu, lens)
    with pytest.raises(err, match=r"v_new must be 3-D \[T,H,D\]"):
        f(kn, kn[None], k, k, cu, lens)
    with pytest.raises(err, match=r"v_new must be \[T,H,D\] like k_new"):
        f(kn, _t((31, 2, 64)), k, k, cu, lens)
    with pytest.raises(err, match="k_new and the caches must agree in heads_kv"):
        f(kn, kn, _t((2, 4, 128, 64)), _t((2, 4, 128, 64)), cu, lens)
    with pytest.raises(err, match="kv_lens is required"):
        f(kn, kn, k, k, cu, None)
    with pytest.raises(err, match="cu_seqlens is required"):
        f(kn, kn, k, k, None, lens)
    with pytest.raises(err, match=r"cu_seqlens must be a contiguous \[B \+ 1 = 3\] tensor"):
        f(kn, kn, k, k, _i32(0, 10, 20, 30), lens)
    with pytest.raises(err, match="k_new must be a device tensor"):
        f(kn, kn, k, k, cu, lens)
    with pytest.raises(err, match="block_table is required"):
        fp(kn, kn, k, k, None, cu, lens)
    # B is the table's row count: three sequences, two lengths
    with pytest.raises(err, match=r"kv_lens must be a contiguous \[B\] tensor"):
        fp(kn, kn, k, k, torch.zeros((3, 3), dtype=torch.int32), _i32(0, 1, 2, 3), lens)


def test_torch_ops_registered_with_the_full_schema():
    import fa_mi355x.torch_op as top

    tail = "Tensor? k_scale=None, Tensor? v_scale=None) -> "
    for op, sig in (
            (top.prefill_varlen, "Tensor q, Tensor k_cache, Tensor v_cache, Tensor cu_seqlens_q, "
                                 "Tensor? kv_lens=None, bool causal=True, " + tail + "Tensor"),
            (top.prefill_varlen_paged, "Tensor q, Tensor k_pages, Tensor v_pages, Tensor block_table, "
                                       "Tensor cu_seqlens_q, Tensor? kv_lens=None, bool causal=True, "
                                       + tail + "Tensor"),
            (top.cache_append_varlen, "Tensor cu_seqlens, Tensor kv_lens, " + tail + "()"),
            (top.cache_append_varlen_paged, "Tensor block_table, Tensor cu_seqlens, Tensor kv_lens, "
                                            + tail + "()")):
        schema = str(op.default._schema)
        assert sig in schema, schema
    q, k, cu = _t((20, 2, 64)), _t((1, 2, 64, 64)), _i32(0, 20)
    table = torch.zeros((1, 1), dtype=torch.int32)
    with pytest.raises(ValueError, match="prefill_varlen needs GPU tensors"):
        top.prefill_varlen(q, k, k, cu)
    with pytest.raises(ValueError, match="prefill_varlen_paged needs GPU tensors"):
        top.prefill_varlen_paged(q, k, k, table, cu)
    with pytest.raises(ValueError, match="cache_append_varlen needs GPU tensors"):
        top.cache_append_varlen(q, q, k, k, cu, _i32(20))
    with pytest.raises(ValueError, match="cache_append_varlen_paged needs GPU tensors"):
        top.cache_append_varlen_paged(q, q, k, k, table, cu, _i32(20))
    from torch._subclasses.fake_tensor import FakeTensorMode

    with FakeTensorMode():
        fq = torch.empty((600, 8, 128), dtype=torch.bfloat16)
        fk = torch.empty((5, 2, 576, 128), dtype=torch.bfloat16)
        fcu = torch.empty((6,), dtype=torch.int32)
        assert top.prefill_varlen(fq, fk, fk, fcu).shape == fq.shape
        assert top.prefill_varlen_paged(fq, fk, fk, torch.empty((5, 9), dtype=torch.int32), fcu).shape == fq.shape


# ---- compile-time resources ----------------------------------------------------------

PRE_UNITS = ["fa_prefill_varlen.hip", "fa_prefill_varlen_paged.hip", "fa_prefill_varlen_kv8.hip",
             "fa_prefill_varlen_paged_kv8.hip"]


def test_kernel_resource_usage():
    """The budget of the padded kernels holds for every packed instantiation: no
    scratch, the prefill kernels' one LDS constant, no LDS in append."""
    src = open(os.path.join(cc.PKG, "csrc", "fa_prefill_kernel.hpp")).read()
    lds_max = int(re.findall(r"constexpr int kPrefillLdsBytes = (\d+);", src)[0])
    assert lds_max == 65536
    usage = cc.kernel_resource_usage(PRE_UNITS + ["fa_cache_append_varlen.hip"])
    for unit, kernels in zip(PRE_UNITS, usage):
        mine = [x for x in kernels if "fa_prefill_kernel" in x[0]]
        assert len(mine) == 4 and all("PrefillPacked" in x[0] for x in mine), (unit, [x[0] for x in kernels])
        for name, scratch, lds in mine:
            print(f"{unit} {name}: scratch {scratch} LDS {lds}")
            assert scratch == 0, (unit, name, scratch)
            assert lds == lds_max, (unit, name, lds)
    mine = [x for x in usage[-1] if "fa_cache_append_kernel" in x[0]]
    # {16-bit copy, f16 -> FP8, bf16 -> FP8} x {contiguous, paged} x {128, 64}
    assert len(mine) == 12 and all("PackedSrc" in x[0] for x in mine), [x[0] for x in usage[-1]]
    for name, scratch, lds in mine:
        print(f"fa_cache_append_varlen.hip {name}: scratch {scratch} LDS {lds}")
        assert scratch == 0 and lds == 0, (name, scratch, lds)
