"""MLA sparse attention (fa_mi355x.flash_attention_mla_sparse) on the GPU
against a plain float64 gather-and-softmax of include/fa_mi355x_mla_sparse.h's
contract on the same rounded 16-bit inputs.  The pool has 1001 rows and every
odd one is NaN: valid entries name even rows only (rows 0 and 1000 among
them), so a row index off by one or a read outside a list turns the output
NaN.  Four tokens: distinct rows; holes scattered through the list (-1, R,
2^31 - 1, -2^31; the whole first tile when topk > 64); five rows drawn with
replacement; holes only."""
import functools
import math

import numpy as np
import pytest
import torch

import decode_refs as dr
import fa_mi355x as fa

gpu = pytest.mark.gpu
DEV = dr.DEV
N, R, DQK, DV = 4, 1001, 576, 512
HQS = [1, 16, 24, 80, 128]   # narrow partial, narrow full, wide partial, a partial second group, two full groups
TOPKS = [1, 65, 192, 320]    # one entry, a ragged second tile, an odd tile count, more tiles than any split
HOLES = (-1, R, 2 ** 31 - 1, -2 ** 31)
SCALES = (1 / math.sqrt(192), 0.1147)
GATES = {torch.float16: dr.GATE_F16, torch.bfloat16: dr.GATE_BF16}
MATRIX = [pytest.mark.parametrize("ns", [0, 1, 3]),
          pytest.mark.parametrize("topk", TOPKS),
          pytest.mark.parametrize("dtype", dr.DTYPES)]


def matrix(test):
    for mark in MATRIX:
        test = mark(test)
    return test


def scale_of(hq, topk):
    return SCALES[(HQS.index(hq) + TOPKS.index(topk)) & 1]


def f64(t):
    return t.detach().float().cpu().numpy().astype(np.float64)


@functools.lru_cache(maxsize=None)
def host_inputs(dtype, hq):
    """Seeded 16-bit (q [N,Hq,576], pool [R,576]) of magnitude <= 1 on the CPU, the pool's odd rows NaN."""
    gen = torch.Generator().manual_seed(7000 + hq)
    q, pool = ((torch.rand(shape, generator=gen) * 2 - 1).to(dtype) for shape in ((N, hq, DQK), (R, DQK)))
    dr.nan_fill(pool[1::2])
    return q, pool


@functools.lru_cache(maxsize=None)
def lists(topk):
    """int32 [N, topk]: the four tokens' index lists (see the module's text)."""
    rng = np.random.default_rng(topk)
    inner = np.arange(2, R - 1, 2)  # rows 0 and 1000 are placed below
    idx = np.stack([rng.permutation(inner)[:topk], rng.permutation(inner)[:topk],
                    rng.choice(np.array([0, 1000, 2, 500, 998]), topk), np.resize(HOLES, topk)]).astype(np.int64)
    pos = np.arange(topk)
    holes = (pos % 3 == 1) | ((pos < 64) & (topk > 64))
    idx[1, holes] = np.resize(HOLES, int(holes.sum()))
    idx[0, 0], idx[1, -1], idx[2, -1] = 1000, 0, 1000
    if topk > 1:
        idx[0, -1], idx[2, 0] = 0, 0
    return idx.astype(np.int32)


def contract_f64(q, pool, idx, scale):
    """(O [N,Hq,512], LSE [N,Hq], max |s|) of the header's contract in float64."""
    n, hq, _ = q.shape
    o, lse, smax = np.zeros((n, hq, DV)), np.full((n, hq), -np.inf), 0.0
    for t in range(n):
        rows = pool[idx[t][(idx[t] >= 0) & (idx[t] < len(pool))]]
        if len(rows):
            s = scale * q[t] @ rows.T  # [Hq, valid]
            smax = max(smax, float(np.abs(s).max()))
            mx = s.max(-1, keepdims=True)
            p = np.exp(s - mx)
            o[t] = p @ rows[:, :DV] / p.sum(-1, keepdims=True)
            lse[t] = mx[:, 0] + np.log(p.sum(-1))
    return o, lse, smax


@functools.lru_cache(maxsize=None)
def reference(dtype, hq, topk):
    q, pool = host_inputs(dtype, hq)
    return contract_f64(f64(q), f64(pool), lists(topk), scale_of(hq, topk))


def check(o, lse, ref, dtype, what):
    ro, rl, smax = ref
    assert o.dtype == dtype and o.shape == ro.shape and bool(torch.isfinite(o).all()), what
    err = float(np.abs(f64(o) - ro).max())
    print(f"{what}: max_abs_diff {err:.3e}")
    assert err <= GATES[dtype], (what, err)
    dr.check_lse(lse, rl, smax, what)
    assert int(torch.count_nonzero(o.cpu()[torch.from_numpy(np.isneginf(rl))])) == 0, what


def test_rounding_alone_does_not_pass_the_gate():
    """No GPU: the float64 reference rounded to each output type sits within
    half of each gate on every input below (|O| <= max |ckv| <= 1, a convex
    combination), so a gate is not met by rounding alone."""
    for dtype, gate in GATES.items():
        for hq in HQS:
            for topk in TOPKS:
                ro = reference(dtype, hq, topk)[0]
                assert np.isfinite(ro).all() and np.abs(ro).max() <= 1
                assert np.abs(f64(torch.from_numpy(ro).to(dtype)) - ro).max() <= gate / 2


@gpu
@pytest.mark.parametrize("hq", HQS)
@matrix
def test_contract(dtype, topk, ns, hq):
    q, pool = (t.to(DEV) for t in host_inputs(dtype, hq))
    idx = torch.from_numpy(lists(topk)).to(DEV)
    what = f"{dr.name(dtype)} h{hq} topk{topk} ns{ns}"
    o, lse = fa.flash_attention_mla_sparse(q, pool, idx, softmax_scale=scale_of(hq, topk), return_lse=True,
                                           num_splits=ns)
    check(o, lse, reference(dtype, hq, topk), dtype, what)
    assert bool(torch.isneginf(lse[3]).all()), what  # holes only: O = 0 exactly (checked above), LSE = -inf
    if ns > 1:
        assert dr.ws_counters_zero(), what


@gpu
@pytest.mark.parametrize("hq", [16, 80])
@matrix
def test_entry_census(dtype, topk, ns, hq):
    """q = 0: every score is 0, so LSE = ln(valid entries, duplicates counted)
    exactly; the even rows are 1 in the value dims and 1/2 in the other 64, so
    O = 1 on every token with a valid entry."""
    q = torch.zeros((N, hq, DQK), dtype=dtype, device=DEV)
    pool = torch.ones((R, DQK), dtype=dtype)
    pool[:, DV:] = 0.5
    dr.nan_fill(pool[1::2])
    idx = lists(topk)
    o, lse = fa.flash_attention_mla_sparse(q, pool.to(DEV), torch.from_numpy(idx).to(DEV),
                                           softmax_scale=scale_of(hq, topk), return_lse=True, num_splits=ns)
    count = np.broadcast_to(((idx >= 0) & (idx < R)).sum(-1)[:, None], (N, hq)).astype(np.float64)
    what = f"census {dr.name(dtype)} h{hq} topk{topk} ns{ns}"
    with np.errstate(divide="ignore"):
        dr.check_lse(lse, np.log(count), 0.0, what)
    want = torch.from_numpy((count > 0).astype(np.float32))[..., None].expand(-1, -1, DV)
    assert float((o.float().cpu() - want).abs().max()) <= torch.finfo(dtype).eps, what
    assert int(torch.count_nonzero(o.cpu()[want == 0])) == 0, what


@gpu
@pytest.mark.parametrize("ns", [1, 3])
@pytest.mark.parametrize("hq", [16, 128])
@pytest.mark.parametrize("dtype", dr.DTYPES)
def test_bit_identities(dtype, hq, ns):
    """Two calls give the same bits; the 4-D form equals the 3-D form; the torch op equals the function."""
    import fa_mi355x.torch_op_mla_sparse as tos

    topk = 192
    q, pool = (t.to(DEV) for t in host_inputs(dtype, hq))
    idx = torch.from_numpy(lists(topk)).to(DEV)
    kw = dict(softmax_scale=SCALES[0], return_lse=True, num_splits=ns)
    first = fa.flash_attention_mla_sparse(q, pool, idx, **kw)
    assert dr.same(first, fa.flash_attention_mla_sparse(q, pool, idx, **kw))
    o4, lse4 = fa.flash_attention_mla_sparse(q.view(2, 2, hq, DQK), pool.view(7, 143, DQK), idx.view(2, 2, topk), **kw)
    assert o4.shape == (2, 2, hq, DV) and lse4.shape == (2, 2, hq)
    assert dr.same(first, (o4.view(N, hq, DV), lse4.view(N, hq)))
    assert torch.equal(tos.sparse(q, pool, idx, SCALES[0]),
                       fa.flash_attention_mla_sparse(q, pool, idx, softmax_scale=SCALES[0]))


@gpu
@pytest.mark.parametrize("dtype", dr.DTYPES)
def test_pool_past_4gib(dtype):
    """A 4.38-GB pool of which only the listed rows are written: rows below
    2^32 / 1152 and the pool's last rows, R - 1 among them, in one list."""
    rows, hq, topk = 3_800_000, 16, 65
    rng = np.random.default_rng(5)
    listed = np.unique(np.concatenate([rng.choice(3_700_000, 40, replace=False), np.arange(rows - 25, rows)]))
    assert len(listed) == topk and listed[0] < 2 ** 32 // 1152 < listed[-1] == rows - 1
    idx = np.stack([rng.permutation(listed), rng.permutation(listed)])
    gen = torch.Generator().manual_seed(11)
    q, vals = ((torch.rand(shape, generator=gen) * 2 - 1).to(dtype) for shape in ((2, hq, DQK), (topk, DQK)))
    pool = torch.empty((rows, DQK), dtype=dtype, device=DEV)
    pool[torch.from_numpy(listed).to(DEV)] = vals.to(DEV)
    o, lse = fa.flash_attention_mla_sparse(q.to(DEV), pool, torch.from_numpy(idx.astype(np.int32)).to(DEV),
                                           softmax_scale=SCALES[0], return_lse=True)
    check(o, lse, contract_f64(f64(q), f64(vals), np.searchsorted(listed, idx), SCALES[0]), dtype,
          f"4gib {dr.name(dtype)}")
