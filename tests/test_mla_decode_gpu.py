"""MLA decode (fa_mi355x.flash_attention_mla_decode[_paged]) on the GPU against
a plain float64 restatement of include/fa_mi355x_mla.h's contract, on the same
rounded 16-bit inputs: B = 3, capacity 320, cache rows at or past each length
NaN, spare pool pages NaN and table entries past the length junk ids."""
import functools
import math

import numpy as np
import pytest
import torch

import decode_refs as dr
import fa_mi355x as fa

gpu = pytest.mark.gpu
DEV = dr.DEV
B, CAP, DQK, DV = 3, 320, 576, 512
GEOMS = [(1, 1), (16, 1), (5, 3), (3, 7), (16, 2), (64, 1), (24, 3), (128, 1)]  # (Hq, Sq)
FORMS = [pytest.param(0, id="contig"), pytest.param(64, id="page64"), pytest.param(128, id="page128")]
SCALES = (1 / math.sqrt(192), 0.1147)
GATES = {torch.float16: dr.GATE_F16, torch.bfloat16: dr.GATE_BF16}
MATRIX = [pytest.mark.parametrize("geom", GEOMS, ids=lambda g: "h%ds%d" % g),
          pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"]),
          pytest.mark.parametrize("ns", [0, 1, 2, 3]),
          pytest.mark.parametrize("psz", FORMS),
          pytest.mark.parametrize("dtype", dr.DTYPES)]


def matrix(test):
    for mark in MATRIX:
        test = mark(test)
    return test


def triples(sq):
    return ((max(sq - 2, 0), sq, sq + 1), (0, 64, 64 + sq // 2), (65, 128 + sq // 2, 259))


def scale_of(geom, causal):
    return SCALES[(GEOMS.index(geom) + causal) & 1]


def f64(t):
    return t.detach().float().cpu().numpy().astype(np.float64)


@functools.lru_cache(maxsize=None)
def host_inputs(dtype, hq, sq):
    """Seeded 16-bit (q, ckv) of magnitude <= 1 on the CPU (read-only)."""
    gen = torch.Generator().manual_seed(1000 * hq + sq)
    return tuple((torch.rand(shape, generator=gen) * 2 - 1).to(dtype) for shape in ((B, hq, sq, DQK), (B, CAP, DQK)))


def visible(lens, sq, causal):
    """[B, Sq]: keys row t of element b sees (a prefix of the cache)."""
    n = np.asarray(lens)[:, None]
    return np.clip(np.minimum(n, n - sq + 1 + np.arange(sq)[None, :]) if causal else n + 0 * np.arange(sq), 0, None)


def contract_f64(q, c, lens, causal, scale):
    """(O [B,Hq,Sq,512], LSE [B,Hq,Sq], max |s|) of the header's contract in float64."""
    b, hq, sq, _ = q.shape
    o, lse, smax = np.zeros((b, hq, sq, DV)), np.full((b, hq, sq), -np.inf), 0.0
    vis = visible(lens, sq, causal)
    for bi in range(b):
        for t in range(sq):
            n = int(vis[bi, t])
            if n == 0:
                continue
            s = scale * q[bi, :, t] @ c[bi, :n].T  # [Hq, n]
            smax = max(smax, float(np.abs(s).max()))
            mx = s.max(-1, keepdims=True)
            p = np.exp(s - mx)
            o[bi, :, t] = p @ c[bi, :n, :DV] / p.sum(-1, keepdims=True)
            lse[bi, :, t] = mx[:, 0] + np.log(p.sum(-1))
    return o, lse, smax


@functools.lru_cache(maxsize=None)
def reference(dtype, hq, sq, lens, causal, scale):
    q, c = host_inputs(dtype, hq, sq)
    return contract_f64(f64(q), f64(c), lens, causal, scale)


def device_cache(c, lens, psz):
    """(cache, None) or (pool, table) on the device from the host cache [B,CAP,576]."""
    c = c.clone()
    for bi, n in enumerate(lens):
        dr.nan_fill(c[bi, n:])
    if not psz:
        return c.to(DEV), None
    pad = dr.nan_fill(torch.empty((B, -(-CAP // psz) * psz, DQK), dtype=c.dtype))
    pad[:, :CAP] = c
    pool, _, table = dr.paginate(pad[:, None], pad[:, None], psz, lens, seed=3, filler="junk")
    return pool[:, 0].contiguous().to(DEV), table.to(DEV)


def call(q, cache, table, lens, **kw):
    if table is None:
        return fa.flash_attention_mla_decode(q, cache, dr.lens(lens), return_lse=True, **kw)
    return fa.flash_attention_mla_decode_paged(q, cache, table, dr.lens(lens), return_lse=True, **kw)


def test_rounding_alone_does_not_pass_the_gate():
    """The float64 reference rounded to each output type sits within half of
    each gate (|O| <= max |c| <= 1), so a gate is not met by rounding alone."""
    for dtype, gate in GATES.items():
        for hq, sq in GEOMS:
            for causal in (False, True):
                for lens in triples(sq):
                    ro = reference(dtype, hq, sq, lens, causal, scale_of((hq, sq), causal))[0]
                    assert np.abs(f64(torch.from_numpy(ro).to(dtype)) - ro).max() <= gate / 2


@gpu
@matrix
def test_contract(dtype, psz, ns, causal, geom):
    hq, sq = geom
    scale = scale_of(geom, causal)
    q, c = host_inputs(dtype, hq, sq)
    for lens in triples(sq):
        what = f"{dr.name(dtype)} page{psz} ns{ns} causal{causal} h{hq}s{sq} {lens}"
        ro, rl, smax = reference(dtype, hq, sq, lens, causal, scale)
        o, lse = call(q.to(DEV), *device_cache(c, lens, psz), lens, softmax_scale=scale, causal=causal,
                      num_splits=ns)
        assert o.shape == (B, hq, sq, DV) and o.dtype == dtype and bool(torch.isfinite(o).all()), what
        err = float(np.abs(f64(o) - ro).max())
        print(f"{what}: max_abs_diff {err:.3e}")
        assert err <= GATES[dtype], (what, err)
        dr.check_lse(lse, rl, smax, what)
        assert int(torch.count_nonzero(o.cpu()[torch.from_numpy(np.isneginf(rl))])) == 0, what
        if ns > 1:
            assert dr.ws_counters_zero(), what


@gpu
@matrix
def test_key_census(dtype, psz, ns, causal, geom):
    """q = 0: every score is 0, so LSE = ln(visible keys) exactly; the cache is
    1 in the value dims and 1/2 in the other 64, so O = 1 on every row that
    sees a key: the value slice is dims 0..511 and the normalisation is right."""
    hq, sq = geom
    q = torch.zeros((B, hq, sq, DQK), dtype=dtype, device=DEV)
    c = torch.ones((B, CAP, DQK), dtype=dtype)
    c[..., DV:] = 0.5
    for lens in triples(sq):
        what = f"census {dr.name(dtype)} page{psz} ns{ns} causal{causal} h{hq}s{sq} {lens}"
        o, lse = call(q, *device_cache(c, lens, psz), lens, softmax_scale=scale_of(geom, causal), causal=causal,
                      num_splits=ns)
        n = np.broadcast_to(visible(lens, sq, causal)[:, None, :], (B, hq, sq)).astype(np.float64)
        with np.errstate(divide="ignore"):
            dr.check_lse(lse, np.log(n), 0.0, what)
        want = torch.from_numpy((n > 0).astype(np.float32))[..., None].expand(-1, -1, -1, DV)
        assert float((o.float().cpu() - want).abs().max()) <= torch.finfo(dtype).eps, what
        assert int(torch.count_nonzero(o.cpu()[want == 0])) == 0, what


@gpu
@pytest.mark.parametrize("ns", [1, 3])
@pytest.mark.parametrize("geom", [(16, 1), (24, 3)], ids=lambda g: "h%ds%d" % g)
@pytest.mark.parametrize("dtype", dr.DTYPES)
def test_bit_identities(dtype, geom, ns):
    """Paged equals contiguous on the gathered cache at equal num_splits, for
    pages of 64 and 128 and a shuffled table; two calls give the same bits."""
    hq, sq = geom
    q, c = host_inputs(dtype, hq, sq)
    q, lens = q.to(DEV), triples(sq)[2]
    kw = dict(softmax_scale=SCALES[0], causal=True, num_splits=ns)
    for psz in (64, 128):
        pool, table = device_cache(c, lens, psz)
        paged = call(q, pool, table, lens, **kw)
        assert dr.same(paged, call(q, pool, table, lens, **kw))
        gathered = dr.gather(pool[:, None], table)[:, 0].contiguous()
        assert dr.same(paged, call(q, gathered, None, lens, **kw)), psz


@gpu
def test_graph_replay_follows_kv_lens():
    hq, sq = 24, 3
    q, c = (t.to(DEV) for t in host_inputs(torch.float16, hq, sq))
    kl = dr.lens((65, 130, 259))
    kw = dict(softmax_scale=SCALES[1], causal=True, num_splits=2, return_lse=True)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        fa.flash_attention_mla_decode(q, c, kl, **kw)  # warm-up outside the capture
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            res = fa.flash_attention_mla_decode(q, c, kl, **kw)
    torch.cuda.current_stream().wait_stream(stream)
    for lens in ((3, 64, 320), (65, 130, 259), (0, 200, 1)):
        kl.copy_(dr.lens(lens))
        graph.replay()
        torch.cuda.synchronize()
        assert dr.same(res, fa.flash_attention_mla_decode(q, c, dr.lens(lens), **kw)), lens
        ro, rl, smax = reference(torch.float16, hq, sq, lens, True, SCALES[1])
        assert float(np.abs(f64(res[0]) - ro).max()) <= dr.GATE_F16
        dr.check_lse(res[1], rl, smax, f"graph {lens}")


@gpu
@pytest.mark.parametrize("psz", [0, 64], ids=["decode", "decode_paged"])
def test_torch_ops_equal_the_functions(psz):
    import fa_mi355x.torch_op_mla as tom

    hq, sq = 16, 2
    q, c = host_inputs(torch.bfloat16, hq, sq)
    lens = triples(sq)[2]
    q, kl = q.to(DEV), dr.lens(lens)
    cache, table = device_cache(c, lens, psz)
    if psz:
        got = tom.decode_paged(q, cache, table, SCALES[0], kl, False)
    else:
        got = tom.decode(q, cache, SCALES[0], kl, False)
    want = call(q, cache, table, lens, softmax_scale=SCALES[0], causal=False)[0]
    assert torch.equal(got, want) and got.shape == (B, hq, sq, DV)
