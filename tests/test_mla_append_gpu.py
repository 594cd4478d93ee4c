"""The writers of the MLA caches on the GPU against the torch expressions on the
CPU, byte for byte: fa_mi355x.flash_attention_mla_append[_paged] over the four
latent cache forms and flash_attention_mla_indexer_append.  Every destination
is prefilled with a sentinel and compared whole, which shows both what is
written and that nothing else is.  The kernel's token block is 16; capacity 128
(two pages of 64), rope_len 132.

  RAGGED  n_b = 0 | 1 | 15 (positions 55..69: across the page edge) | 17 | 20
          (positions 115..134: past the capacity from 128, past the tables from
          132) | 5 (positions -2..2) | 6 (paged: its page ids lie outside the pool)
  UNIFORM four sequences of 17: positions 0..16 | 53..69 | 118..134 | 34..50
          (paged: outside the pool)
"""
import functools

import pytest
import torch

import decode_refs as dr
import fa_mi355x as fa
import fp8_contract

gpu, DEV = pytest.mark.gpu, dr.DEV
CAP, PAGE, ROPE_LEN, HQ = 128, 64, 132, 11
RAGGED = ((0, 1, 15, 17, 20, 5, 6), (5, 1, 70, 17, 135, 3, 40), True)
UNIFORM = ((17, 17, 17, 17), (17, 70, 135, 51), False)
DECODE = ((1, 1, 1), (1, 64, 129), False)
FORMS = [(paged, kv8) for paged in (False, True) for kv8 in (False, True)]
SENT16, SENT8 = 7.0, 0x55


def rope(x, c, s, inter):
    a, b = (x[..., 0::2], x[..., 1::2]) if inter else (x[..., :32], x[..., 32:])
    a, b = a.float(), b.float()
    ra, rb = (a * c - b * s).to(x.dtype), (b * c + a * s).to(x.dtype)
    return torch.stack((ra, rb), -1).flatten(-2) if inter else torch.cat((ra, rb), -1)


@functools.lru_cache(maxsize=None)
def sources(dtype, total):
    """Seeded CPU tensors: kv_a [T, 584] (c_kv | k_pe | 8 spare), q [T, HQ, 192], the tables, an index key [T, 128]."""
    gen = torch.Generator().manual_seed(total)
    kv_a, q, k = (torch.randn(s, generator=gen).mul(2).to(dtype) for s in ((total, 584), (total, HQ, 192), (total, 128)))
    ang = torch.rand((ROPE_LEN, 32), generator=gen) * 6.28
    return kv_a, q, ang.cos().contiguous(), ang.sin().contiguous(), k


def rows_of(case, paged):
    """Per token (b, pos) and the flat pool row it lands in (-1: dropped by capacity or page), the table, pool pages."""
    ns, lens, _ = case
    b = torch.repeat_interleave(torch.arange(len(ns)), torch.tensor(ns))
    t = torch.cat([torch.arange(n) for n in ns])
    pos = torch.tensor(lens)[b] - torch.tensor(ns)[b] + t
    npages = 2 * len(ns) + 1
    table = torch.randperm(npages, generator=torch.Generator().manual_seed(1))[:2 * len(ns)].view(len(ns), 2)
    table[-1] = torch.tensor([npages, -1])  # the last sequence: outside the pool
    ok = (pos >= 0) & (pos < CAP)
    pc = pos.clamp(0, CAP - 1)
    if paged:
        page = table[b, pc // PAGE]
        ok &= (page >= 0) & (page < npages)
        row = page * PAGE + pc % PAGE
    else:
        row = b * CAP + pc
    return pos, torch.where(ok, row, -1), table.to(torch.int32), npages


def run_append(case, dtype, paged, kv8, inter, scale=None, tables=True, hq=HQ, inplace=False, decode_layout=False):
    """One launch on sentinel-filled destinations; returns (cache, q buffer) from the GPU and as expected."""
    ns, lens, ragged = case
    total = sum(ns)
    kv_a, q, cos, sin, _ = sources(dtype, total)
    pos, row, table, npages = rows_of(case, paged)
    s = 1.0 if scale is None else scale
    # the expectation
    seen = (pos >= 0) & (pos < ROPE_LEN) if tables else torch.ones_like(pos, dtype=torch.bool)
    c, sn = (cos[pos.clamp(0, ROPE_LEN - 1)], sin[pos.clamp(0, ROPE_LEN - 1)]) if tables else (None, None)
    kpe = rope(kv_a[:, 512:576], c, sn, inter) if tables else kv_a[:, 512:576]
    latent = torch.cat((kv_a[:, :512], kpe), -1)
    nrows = npages * PAGE if paged else len(ns) * CAP
    if kv8:
        want_c = torch.full((nrows, 576), SENT8, dtype=torch.uint8)
        latent = fp8_contract.torch_reference_bytes(latent, s)
    else:
        want_c = torch.full((nrows, 576), SENT16, dtype=dtype)
    w = seen & (row >= 0)
    want_c[row[w]] = latent[w]
    qbuf = torch.full((total, HQ, 584), SENT16, dtype=dtype)
    qbuf[..., :512] = q[..., :1].expand(-1, -1, 512)  # the caller's absorbed q_nope: must survive
    if inplace:
        qbuf[..., 512:576] = q[..., 128:]
    want_q = qbuf.clone()
    if hq:
        want_q[seen, :hq, 512:576] = rope(q[seen, :hq, 128:], c[seen, None], sn[seen, None], inter)
    # the launch
    cache = want_c.new_full(want_c.shape, SENT8 if kv8 else SENT16).view(-1, PAGE if paged else CAP, 576).to(DEV)
    dq, dkv = qbuf.to(DEV), kv_a.to(DEV)
    q_out = dq[:, :hq, :576]
    q_pe = q_out[..., 512:] if inplace else q.to(DEV)[:, :hq, 128:]
    args = dict(cu_seqlens=torch.tensor([0] + list(ns), dtype=torch.int32).cumsum(0).int().to(DEV) if ragged else None,
                q_pe=q_pe if hq else None, q_out=(q_out.unsqueeze(2) if decode_layout else q_out) if hq else None,
                cos=cos.to(DEV) if tables else None, sin=sin.to(DEV) if tables else None, interleaved=inter,
                ckv_scale=None if scale is None else torch.tensor([scale], dtype=torch.float32, device=DEV))
    kv_lens = torch.tensor(lens, dtype=torch.int32, device=DEV)
    if paged:
        fa.flash_attention_mla_append_paged(dkv[:, :512], dkv[:, 512:576], cache, table.to(DEV), kv_lens, **args)
    else:
        fa.flash_attention_mla_append(dkv[:, :512], dkv[:, 512:576], cache, kv_lens, **args)
    torch.cuda.synchronize()
    return cache.cpu().view(-1, 576), want_c, dq.cpu(), want_q


def same_bits(got, want):
    assert got.shape == want.shape and got.dtype == want.dtype
    bits = torch.uint8 if got.element_size() == 1 else torch.int16
    bad = (got.view(bits) != want.view(bits)).nonzero()
    assert bad.numel() == 0, (len(bad), bad[:4].tolist())


@gpu
@pytest.mark.parametrize("case", [RAGGED, UNIFORM], ids=["ragged", "uniform"])
@pytest.mark.parametrize("inter", [False, True])
@pytest.mark.parametrize("paged,kv8", FORMS)
@pytest.mark.parametrize("dtype", dr.DTYPES)
def test_latent_append(dtype, paged, kv8, inter, case):
    cache, want_c, q, want_q = run_append(case, dtype, paged, kv8, inter, scale=0.75 if kv8 and inter else None)
    same_bits(cache, want_c)
    same_bits(q, want_q)


@gpu
@pytest.mark.parametrize("kw", [dict(inplace=True), dict(tables=False, hq=0), dict(case=DECODE, decode_layout=True)],
                         ids=["inplace_q", "plain", "decode_step"])
@pytest.mark.parametrize("paged,kv8", FORMS)
@pytest.mark.parametrize("dtype", dr.DTYPES)
def test_latent_append_variants(dtype, paged, kv8, kw):
    kw = {"case": RAGGED, **kw}
    cache, want_c, q, want_q = run_append(kw.pop("case"), dtype, paged, kv8, False, scale=1.5 if kv8 else None, **kw)
    same_bits(cache, want_c)
    same_bits(q, want_q)


def act_quant(x, pow2):
    """DeepSeek-V3.2's act_quant per row of the 16-bit CPU tensor x: (bytes, scales)."""
    s = x.float().abs().amax(-1).clamp_min(1e-4) / 448.0
    if pow2:
        m, e = torch.frexp(s)
        s = torch.where(m == 0.5, s, torch.ldexp(torch.ones_like(s), e))
    return torch.stack([fp8_contract.torch_reference_bytes(r, v.item()) for r, v in zip(x, s)]), s


@gpu
@pytest.mark.parametrize("pow2", [False, True])
@pytest.mark.parametrize("paged", [False, True])
@pytest.mark.parametrize("dtype", dr.DTYPES)
def test_indexer_append(dtype, paged, pow2):
    ns, lens, _ = RAGGED
    k = sources(dtype, sum(ns))[4].clone()
    # tokens 16..19 (written rows of the fourth sequence): zeros (the 1e-4 floor); amax / 448 = 2^-3 exactly;
    # one ulp above it; the type's largest finite magnitude
    k[16] = 0
    k[17:19] = k[17:19].clamp(-50, 50)
    k[17, 5], k[18, 5] = -56.0, (torch.tensor([56.0], dtype=dtype).view(torch.int16) + 1).view(dtype)[0]
    k[19, 127] = torch.finfo(dtype).max
    pos, row, table, npages = rows_of(RAGGED, paged)
    nrows = npages * PAGE if paged else len(ns) * CAP
    want_b, want_s = torch.full((nrows, 128), SENT8, dtype=torch.uint8), torch.full((nrows,), -1.0)
    qb, qs = act_quant(k, pow2)
    assert qs[17] == 0.125 and (qs[18] == 0.25 if pow2 else qs[18] > 0.125)
    want_b[row[row >= 0]], want_s[row[row >= 0]] = qb[row >= 0], qs[row >= 0]
    wide = torch.zeros((sum(ns), 136), dtype=dtype)
    wide[:, :128] = k
    pool, scales = torch.full_like(want_b, SENT8).view(-1, PAGE if paged else CAP, 128).to(DEV), torch.full_like(want_s, -1).to(DEV)
    fa.flash_attention_mla_indexer_append(
        wide.to(DEV)[:, :128], pool, torch.tensor(lens, dtype=torch.int32, device=DEV), scales,
        cu_seqlens=torch.tensor([0] + list(ns), dtype=torch.int32).cumsum(0).int().to(DEV),
        block_table=table.to(DEV) if paged else None, scale_pow2=pow2)
    torch.cuda.synchronize()
    same_bits(pool.cpu().view(-1, 128), want_b)
    assert torch.equal(scales.cpu().view(torch.int32), want_s.view(torch.int32))


@gpu
def test_graph_replay_follows_lengths_and_scale():
    """A captured decode-step append, replayed after kv_lens and ckv_scale are rewritten, writes the next rows under
    the new scale; three replays against the CPU expectation."""
    dtype, b = torch.bfloat16, 2
    kv_a, _, cos, sin, _ = sources(dtype, 8)
    cache = torch.full((b, CAP, 576), SENT8, dtype=torch.uint8, device=DEV)
    new, lens = torch.zeros((b, 584), dtype=dtype, device=DEV), torch.zeros(b, dtype=torch.int32, device=DEV)
    scale, dcos, dsin = torch.ones(1, device=DEV), cos.to(DEV), sin.to(DEV)
    call = lambda: fa.flash_attention_mla_append(new[:, :512], new[:, 512:576], cache, lens, cos=dcos, sin=dsin,
                                                 ckv_scale=scale)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        call()  # (lengths of 0: position -1, nothing is written)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    want = torch.full((b, CAP, 576), SENT8, dtype=torch.uint8)
    for step, s in enumerate((0.5, 1.0, 3.0)):
        rows, kv_lens = kv_a[2 * step:2 * step + 2], torch.tensor([step + 1, 64 + step + 1], dtype=torch.int32)
        new.copy_(rows)
        lens.copy_(kv_lens)
        scale.fill_(s)
        graph.replay()
        pos = kv_lens.long() - 1
        latent = torch.cat((rows[:, :512], rope(rows[:, 512:576], cos[pos], sin[pos], False)), -1)
        want[torch.arange(b), pos] = fp8_contract.torch_reference_bytes(latent, s)
        torch.cuda.synchronize()
        same_bits(cache.cpu(), want)
