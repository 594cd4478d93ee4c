"""fa_mi355x.flash_attention_mla_sparse_kv8 on the GPU against a plain float64
gather-and-softmax over scale * float(byte) (no quantisation error in it).  The
pool has 1001 rows of E4M3 codes with |value| <= 1 and every odd row is the NaN
byte 0x7F, so an index off by one or a read outside a list poisons the output.
Four tokens: distinct rows while the even rows last (rows 0 and 1000 among
them); holes (-1, R, 2^31 - 1, -2^31) at every third entry (pairs lose their
even or their odd row alone), over the whole first tile when topk > 64 and over
entries 16..31 of the second when topk >= 128 (one wave's block empty in a live
tile); five rows drawn with replacement; holes only."""
import functools
import itertools
import math

import numpy as np
import pytest
import torch

import decode_refs as dr
import fa_mi355x as fa
import fp8_contract

gpu, DEV = pytest.mark.gpu, dr.DEV
N, R, DQK, DV = 4, 1001, 576, 512
HQS = [1, 16, 24, 128]       # narrow partial, narrow full, wide partial, two row groups
TOPKS = [1, 65, 192, 577]    # one entry, a ragged second tile, an odd tile count, ten tiles
HOLES = (-1, R, 2 ** 31 - 1, -2 ** 31)
SCALES = (1 / math.sqrt(192), 0.1147)  # the softmax scales
CKV_SCALES = [None, 0.75]
GATES = {torch.float16: dr.GATE_F16, torch.bfloat16: dr.GATE_BF16}
MATRIX = [pytest.mark.parametrize("ns", [0, 1, 3]),
          pytest.mark.parametrize("topk", TOPKS),
          pytest.mark.parametrize("dtype", dr.DTYPES)]

matrix = lambda test: functools.reduce(lambda t, mark: mark(t), MATRIX, test)
scale_of = lambda hq, topk: SCALES[(HQS.index(hq) + TOPKS.index(topk)) & 1]
f64 = lambda t: t.detach().float().cpu().numpy().astype(np.float64)
fp32 = lambda s: 1.0 if s is None else float(np.float32(s))
scale_tensor = lambda s: None if s is None else torch.tensor([s], dtype=torch.float32, device=DEV)
call = lambda *a, **kw: fa.flash_attention_mla_sparse_kv8(*a, **kw)


def codes(shape, gen):
    """uint8 E4M3 codes of magnitude <= 1 (0x00..0x38) with a random sign bit."""
    return (torch.randint(0, 0x39, shape, generator=gen) + 128 * torch.randint(0, 2, shape, generator=gen)).to(torch.uint8)


@functools.lru_cache(maxsize=None)
def host_inputs(dtype, hq):
    """Seeded CPU (q [N,Hq,576] of magnitude <= 1, pool bytes [R,576]), the pool's odd rows the NaN byte."""
    gen = torch.Generator().manual_seed(8000 + hq)
    q = (torch.rand((N, hq, DQK), generator=gen) * 2 - 1).to(dtype)
    pool = codes((R, DQK), gen)
    pool[1::2] = 0x7f
    return q, pool


@functools.lru_cache(maxsize=None)
def lists(topk):
    """int32 [N, topk]: the four tokens' index lists (see the module's text)."""
    rng = np.random.default_rng(topk)
    inner = np.arange(2, R - 1, 2)  # rows 0 and 1000 are placed below
    idx = np.stack([np.resize(rng.permutation(inner), topk), np.resize(rng.permutation(inner), topk),
                    rng.choice(np.array([0, 1000, 2, 500, 998]), topk), np.resize(HOLES, topk)]).astype(np.int64)
    pos = np.arange(topk)
    holes = (pos % 3 == 1) | ((pos < 64) & (topk > 64)) | ((pos >= 80) & (pos < 96) & (topk >= 128))
    idx[1, holes] = np.resize(HOLES, int(holes.sum()))
    idx[0, 0], idx[1, -1], idx[2, -1] = 1000, 0, 1000
    if topk > 1:
        idx[0, -1], idx[2, 0] = 0, 0
    return idx.astype(np.int32)


def contract_f64(q, pool, idx, scale):
    """(O [N,Hq,512], LSE [N,Hq], max |s|) of the header's contract in float64 over the dequantised `pool`."""
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
def reference(dtype, hq, topk, ckv_scale):
    q, pool = host_inputs(dtype, hq)
    return contract_f64(f64(q), fp32(ckv_scale) * f64(pool.view(fp8_contract.FP8)), lists(topk), scale_of(hq, topk))


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
    half of each gate on every input below (|O| <= max |c| <= 1)."""
    for (dtype, gate), hq, topk, s in itertools.product(GATES.items(), HQS, TOPKS, CKV_SCALES):
        ro = reference(dtype, hq, topk, s)[0]
        assert np.isfinite(ro).all() and np.abs(ro).max() <= 1
        assert np.abs(f64(torch.from_numpy(ro).to(dtype)) - ro).max() <= gate / 2


@gpu
@pytest.mark.parametrize("ckv_scale", CKV_SCALES)
@pytest.mark.parametrize("hq", HQS)
@matrix
def test_contract(dtype, topk, ns, hq, ckv_scale):
    q, pool = (t.to(DEV) for t in host_inputs(dtype, hq))
    idx = torch.from_numpy(lists(topk)).to(DEV)
    what = f"{dr.name(dtype)} h{hq} topk{topk} ns{ns} scale{ckv_scale}"
    o, lse = call(q, pool, idx, scale_of(hq, topk), scale_tensor(ckv_scale), return_lse=True, num_splits=ns)
    check(o, lse, reference(dtype, hq, topk, ckv_scale), dtype, what)
    assert bool(torch.isneginf(lse[3]).all()), what  # holes only: O = 0 exactly (checked above), LSE = -inf
    if ns > 1:
        assert dr.ws_counters_zero(), what


@gpu
@pytest.mark.parametrize("hq", [16, 128])
@matrix
def test_entry_census(dtype, topk, ns, hq):
    """q = 0: every score is 0, so LSE = ln(valid entries, duplicates counted);
    the even rows are the byte of 1.0 in the value dims and of 0.5 in the other
    64, so O = ckv_scale = 0.75 (exact in both types) on every token with a
    valid entry: the scale reached the value side, once."""
    q = torch.zeros((N, hq, DQK), dtype=dtype, device=DEV)
    pool = torch.full((R, DQK), 0x38, dtype=torch.uint8)  # E4M3 1.0
    pool[:, DV:] = 0x30  # E4M3 0.5
    pool[1::2] = 0x7f
    idx = lists(topk)
    o, lse = call(q, pool.to(DEV), torch.from_numpy(idx).to(DEV), scale_of(hq, topk), scale_tensor(0.75),
                  return_lse=True, num_splits=ns)
    count = np.broadcast_to(((idx >= 0) & (idx < R)).sum(-1)[:, None], (N, hq)).astype(np.float64)
    what = f"census {dr.name(dtype)} h{hq} topk{topk} ns{ns}"
    with np.errstate(divide="ignore"):
        dr.check_lse(lse, np.log(count), 0.0, what)
    want = torch.from_numpy(0.75 * (count > 0).astype(np.float32))[..., None].expand(-1, -1, DV)
    assert float((o.float().cpu() - want).abs().max()) <= torch.finfo(dtype).eps / 2, what  # one ulp below 1
    assert int(torch.count_nonzero(o.cpu()[want == 0])) == 0, what


@gpu
@pytest.mark.parametrize("ns", [1, 3])
@pytest.mark.parametrize("topk", [192, 65])
@pytest.mark.parametrize("hq", [16, 128])
@pytest.mark.parametrize("dtype", dr.DTYPES)
def test_bit_identities(dtype, hq, topk, ns):
    """Two calls give the same bits; the 4-D form equals the 3-D form; the torch
    op equals the function; on the hole-free lists (tokens 0 and 2) the result
    equals the dense kv8 decode on the gathered rows at the same num_splits."""
    import fa_mi355x.torch_op_mla_sparse_kv8 as tos

    q, pool = (t.to(DEV) for t in host_inputs(dtype, hq))
    idx, sc = torch.from_numpy(lists(topk)).to(DEV), scale_tensor(0.75)
    kw = dict(return_lse=True, num_splits=ns)
    first = call(q, pool, idx, SCALES[0], sc, **kw)
    assert dr.same(first, call(q, pool, idx, SCALES[0], sc, **kw))
    o4, lse4 = call(q.view(2, 2, hq, DQK), pool.view(fp8_contract.FP8).view(7, 143, DQK), idx.view(2, 2, topk),
                    SCALES[0], sc, **kw)
    assert o4.shape == (2, 2, hq, DV) and lse4.shape == (2, 2, hq)
    assert dr.same(first, (o4.view(N, hq, DV), lse4.view(N, hq)))
    assert torch.equal(tos.sparse_kv8(q, pool, idx, SCALES[0], sc), call(q, pool, idx, SCALES[0], sc))
    full = [0, 2]
    dense = fa.flash_attention_mla_decode_kv8(q[full][:, :, None], pool[idx[full].long()], ckv_scale=sc,
                                              softmax_scale=SCALES[0], **kw)
    assert dr.same((first[0][full], first[1][full]), (dense[0][:, :, 0], dense[1][:, :, 0]))


@gpu
def test_graph_replay_follows_the_list_and_the_scale():
    hq, topk = 24, 192
    q, pool = (t.to(DEV) for t in host_inputs(torch.float16, hq))
    idx, sc = torch.from_numpy(lists(topk)).to(DEV), scale_tensor(0.75)
    kw = dict(return_lse=True, num_splits=2)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        call(q, pool, idx, SCALES[0], sc, **kw)  # warm-up outside the capture
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            res = call(q, pool, idx, SCALES[0], sc, **kw)
    torch.cuda.current_stream().wait_stream(stream)
    for shift, s in ((0, 0.75), (1, 0.5), (2, 0.5), (0, 0.75)):
        now = torch.from_numpy(np.roll(lists(topk), shift, axis=0).copy()).to(DEV)  # the lists change tokens
        idx.copy_(now)
        sc.fill_(s)
        graph.replay()
        torch.cuda.synchronize()
        assert dr.same(res, call(q, pool, now, SCALES[0], scale_tensor(s), **kw)), (shift, s)


@gpu
@pytest.mark.parametrize("dtype", dr.DTYPES)
def test_pool_past_4gib(dtype):
    """A 4.38-GB pool of which only the listed rows are written: rows below
    2^32 / 576 and the pool's last rows, R - 1 among them, in one list."""
    rows, hq, topk = 7_600_000, 16, 65
    rng = np.random.default_rng(5)
    listed = np.unique(np.concatenate([rng.choice(7_400_000, 40, replace=False), np.arange(rows - 25, rows)]))
    assert len(listed) == topk and listed[0] < 2 ** 32 // 576 < listed[-1] == rows - 1
    idx = np.stack([rng.permutation(listed), rng.permutation(listed)])
    gen = torch.Generator().manual_seed(11)
    q, vals = (torch.rand((2, hq, DQK), generator=gen) * 2 - 1).to(dtype), codes((topk, DQK), gen)
    pool = torch.empty((rows, DQK), dtype=torch.uint8, device=DEV)
    pool[torch.from_numpy(listed).to(DEV)] = vals.to(DEV)
    o, lse = call(q.to(DEV), pool, torch.from_numpy(idx.astype(np.int32)).to(DEV), SCALES[0], scale_tensor(0.75),
                  return_lse=True)
    ref = contract_f64(f64(q), 0.75 * f64(vals.view(fp8_contract.FP8)), np.searchsorted(listed, idx), SCALES[0])
    check(o, lse, ref, dtype, f"4gib {dr.name(dtype)}")
