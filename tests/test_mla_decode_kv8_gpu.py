"""MLA decode over an FP8 latent cache on the GPU against float64 over scale *
float(byte) (include/fa_mi355x_mla_kv8.h; no quantisation error in it): B = 3,
capacity 576 (nine tiles, twice round the four-image ring), rows past a length
and spare pages E4M3 NaN bytes, table entries past the length junk ids."""
import functools
import itertools

import numpy as np
import pytest
import torch

import decode_refs as dr
import fa_mi355x as fa
import fp8_contract

gpu, DEV = pytest.mark.gpu, dr.DEV
B, CAP, DQK, DV = 3, 576, 576, 512
GEOMS = [(1, 1), (16, 1), (5, 3), (16, 2), (64, 1), (24, 3), (128, 1)]  # (Hq, Sq)
FORMS = [pytest.param(0, id="contig"), pytest.param(64, id="page64"), pytest.param(128, id="page128")]
SCALE = 0.1147  # the softmax scale
GATES = {torch.float16: dr.GATE_F16, torch.bfloat16: dr.GATE_BF16}
MATRIX = [pytest.mark.parametrize("geom", GEOMS, ids=lambda g: "h%ds%d" % g),
          pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"]),
          pytest.mark.parametrize("ns", [0, 1, 3]),
          pytest.mark.parametrize("psz", FORMS),
          pytest.mark.parametrize("dtype", dr.DTYPES)]


def matrix(test):
    return functools.reduce(lambda t, mark: mark(t), MATRIX, test)


def triples(sq):
    return ((max(sq - 2, 0), sq, sq + 1), (0, 64, 64 + sq // 2), (65, 259, 575))


f64 = lambda t: t.detach().float().cpu().numpy().astype(np.float64)
fp32 = lambda s: 1.0 if s is None else float(np.float32(s))
scale_tensor = lambda s: None if s is None else torch.tensor([s], dtype=torch.float32, device=DEV)


@functools.lru_cache(maxsize=None)
def host_inputs(dtype, hq, sq, ckv_scale):
    """Seeded CPU (q, bytes), read-only: the cache uniform in (-0.97, 0.97),
    quantised by the cache contract.  Not (-1, 1): from 0.971 / 0.37 on E4M3
    rounds to 2.75, and 2.75 * 0.37 > 1, where bf16's half-ulp passes half its gate."""
    gen = torch.Generator().manual_seed(1000 * hq + sq)
    q, c = ((torch.rand(shape, generator=gen) * 2 - 1) for shape in ((B, hq, sq, DQK), (B, CAP, DQK)))
    return q.to(dtype), fp8_contract.torch_reference_bytes((0.97 * c).to(dtype), fp32(ckv_scale))


def visible(lens, sq, causal):
    n = np.asarray(lens)[:, None]
    return np.clip(np.minimum(n, n - sq + 1 + np.arange(sq)[None, :]) if causal else n + 0 * np.arange(sq), 0, None)


@functools.lru_cache(maxsize=None)
def reference(dtype, hq, sq, lens, causal, ckv_scale, read_scale="same"):
    """(O, LSE, max |s|) of the contract in float64; read_scale: if not the scale written under."""
    q, c8 = host_inputs(dtype, hq, sq, ckv_scale)
    q, c = f64(q), fp32(ckv_scale if read_scale == "same" else read_scale) * f64(c8.view(fp8_contract.FP8))
    o, lse, smax = np.zeros((B, hq, sq, DV)), np.full((B, hq, sq), -np.inf), 0.0
    vis = visible(lens, sq, causal)
    for bi in range(B):
        for t in range(sq):
            n = int(vis[bi, t])
            if n == 0:
                continue
            s = SCALE * q[bi, :, t] @ c[bi, :n].T  # [Hq, n]
            smax = max(smax, float(np.abs(s).max()))
            mx = s.max(-1, keepdims=True)
            p = np.exp(s - mx)
            o[bi, :, t] = p @ c[bi, :n, :DV] / p.sum(-1, keepdims=True)
            lse[bi, :, t] = mx[:, 0] + np.log(p.sum(-1))
    return o, lse, smax


def device_cache(c8, lens, psz):
    """(cache, None) or (pool, table) on the device; whatever holds no live key is E4M3 NaN."""
    c8 = c8.clone()
    for bi, n in enumerate(lens):
        c8[bi, n:] = 0x7f
    if not psz:
        return c8.to(DEV), None
    pad = torch.full((B, -(-CAP // psz) * psz, DQK), 0x7f, dtype=torch.uint8)
    pad[:, :CAP] = c8
    pool, _, table = dr.paginate(pad[:, None], pad[:, None], psz, lens, seed=3, filler="junk")
    return pool[:, 0].contiguous().to(DEV), table.to(DEV)


def call(q, cache, table, lens, **kw):
    kw.update(kv_lens=dr.lens(lens), return_lse=True, softmax_scale=SCALE)
    if table is None:
        return fa.flash_attention_mla_decode_kv8(q, cache, **kw)
    return fa.flash_attention_mla_decode_paged_kv8(q, cache, table, **kw)


def test_rounding_alone_does_not_pass_the_gate():
    """The float64 reference rounded to each output type sits within half of each gate."""
    for (dtype, gate), (hq, sq), causal, s in itertools.product(GATES.items(), GEOMS, (False, True), (None, 0.37)):
        for lens in triples(sq):
            ro = reference(dtype, hq, sq, lens, causal, s)[0]
            assert np.abs(f64(torch.from_numpy(ro).to(dtype)) - ro).max() <= gate / 2


@gpu
@matrix
@pytest.mark.parametrize("ckv_scale", [None, 0.37])
def test_contract(ckv_scale, dtype, psz, ns, causal, geom):
    hq, sq = geom
    q, c8 = host_inputs(dtype, hq, sq, ckv_scale)
    for lens in triples(sq):
        what = f"{dr.name(dtype)} page{psz} ns{ns} causal{causal} h{hq}s{sq} scale{ckv_scale} {lens}"
        ro, rl, smax = reference(dtype, hq, sq, lens, causal, ckv_scale)
        o, lse = call(q.to(DEV), *device_cache(c8, lens, psz), lens, ckv_scale=scale_tensor(ckv_scale),
                      causal=causal, num_splits=ns)
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
    """q = 0: LSE = ln(visible keys); scale 0.5 over bytes of 2.0 in the value
    dims (1.0 in the other 64), so O = 1: the value side carries the scale, once."""
    hq, sq = geom
    q = torch.zeros((B, hq, sq, DQK), dtype=dtype, device=DEV)
    c8 = torch.full((B, CAP, DQK), 0x40, dtype=torch.uint8)  # E4M3 2.0
    c8[..., DV:] = 0x38  # E4M3 1.0
    for lens in triples(sq):
        what = f"census {dr.name(dtype)} page{psz} ns{ns} causal{causal} h{hq}s{sq} {lens}"
        o, lse = call(q, *device_cache(c8, lens, psz), lens, ckv_scale=scale_tensor(0.5), causal=causal,
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
    hq, sq = geom
    q, c8 = host_inputs(dtype, hq, sq, 0.37)
    q, lens = q.to(DEV), triples(sq)[2]
    kw = dict(ckv_scale=scale_tensor(0.37), causal=True, num_splits=ns)
    for psz in (64, 128):
        pool, table = device_cache(c8, lens, psz)
        paged = call(q, pool, table, lens, **kw)
        assert dr.same(paged, call(q, pool, table, lens, **kw))
        gathered = dr.gather(pool[:, None], table)[:, 0].contiguous()
        assert dr.same(paged, call(q, gathered, None, lens, **kw)), psz


@gpu
def test_graph_replay_follows_kv_lens_and_ckv_scale():
    hq, sq = 24, 3
    q, c8 = (t.to(DEV) for t in host_inputs(torch.float16, hq, sq, 0.37))
    kl, sc = dr.lens((65, 130, 259)), scale_tensor(0.37)
    kw = dict(softmax_scale=SCALE, causal=True, num_splits=2, return_lse=True)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        fa.flash_attention_mla_decode_kv8(q, c8, kl, ckv_scale=sc, **kw)  # warm-up outside the capture
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            res = fa.flash_attention_mla_decode_kv8(q, c8, kl, ckv_scale=sc, **kw)
    torch.cuda.current_stream().wait_stream(stream)
    for lens, s in (((3, 64, 576), 0.37), ((65, 130, 259), 0.25), ((0, 200, 1), 0.25), ((65, 130, 259), 0.37)):
        kl.copy_(dr.lens(lens))
        sc.fill_(s)
        graph.replay()
        torch.cuda.synchronize()
        assert dr.same(res, fa.flash_attention_mla_decode_kv8(q, c8, dr.lens(lens), ckv_scale=scale_tensor(s), **kw))
        ro, rl, smax = reference(torch.float16, hq, sq, lens, True, 0.37, s)
        assert float(np.abs(f64(res[0]) - ro).max()) <= dr.GATE_F16, (lens, s)
        dr.check_lse(res[1], rl, smax, f"graph {lens} {s}")


@gpu
@pytest.mark.parametrize("psz", [0, 64], ids=["decode_kv8", "decode_paged_kv8"])
def test_torch_ops_equal_the_functions(psz):
    import fa_mi355x.torch_op_mla_kv8 as tom

    hq, sq = 16, 2
    q, c8 = host_inputs(torch.bfloat16, hq, sq, 0.37)
    lens = triples(sq)[2]
    q, kl, sc = q.to(DEV), dr.lens(lens), scale_tensor(0.37)
    cache, table = device_cache(c8, lens, psz)
    cache = cache.view(torch.float8_e4m3fn)  # the ops and the functions take either dtype
    if psz:
        got = tom.decode_paged_kv8(q, cache, table, SCALE, sc, kl, False)
    else:
        got = tom.decode_kv8(q, cache, SCALE, sc, kl, False)
    want = call(q, cache, table, lens, ckv_scale=sc, causal=False)[0]
    assert torch.equal(got, want) and got.shape == (B, hq, sq, DV)
