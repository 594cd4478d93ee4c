"""GPU tests of cache append (fa_cache_append_* behind
fa_mi355x.flash_attention_cache_append[_paged] and the torch ops): the writer
of the four cache forms the decode entries read.

Every comparison is bit-exact; the feature has no tolerance.  16-bit caches
are compared whole, as int16, with an expectation built by torch indexing on
the CPU over a sentinel fill, so one assertion checks the written rows and
that every other byte is untouched.  FP8 bytes are compared with the torch
expression on the CPU (tests/fp8_contract.py; tests/test_cache_append_cpu.py
pins it against an integer-only model of the contract), never with torch's
device conversion.
Shapes: B = 3, Hkv = 2 (one Hkv = 1 case), cap = 192; paged: page 64, a
3-column table into a permuted pool with two pages no entry names.
"""
import pytest
import torch

import fa_mi355x
from fp8_contract import NAN_PATTERNS, all_patterns, torch_reference_bytes

pytestmark = pytest.mark.gpu

DEV = "cuda"
FP8 = torch.float8_e4m3fn
CAP, PAGE, COLS = 192, 64, 3
SENT16, SENT8 = 0x5a3c, 0x5a
DTYPES = [pytest.param(torch.float16, id="fp16"), pytest.param(torch.bfloat16, id="bf16")]
FORMS = [pytest.param((False, False), id="contig-16"), pytest.param((True, False), id="paged-16"),
         pytest.param((False, True), id="contig-kv8"), pytest.param((True, True), id="paged-kv8")]
# per Sn, the lengths AFTER the append of the three batch elements.  Across the
# cases: a write across a page boundary (65 / 3, 70 / 16, 67 / 67), len = n
# (1 / 1, 16 / 16, 67 / 67), len = cap (192), len < n (0 / 1, 2 / 3, 30 / 67),
# len = 0, len = cap + 5 (197)
LENS = {1: (1, 0, 192), 3: (65, 2, 197), 16: (70, 16, 192), 67: (67, 197, 30)}

append = fa_mi355x.flash_attention_cache_append
append_paged = fa_mi355x.flash_attention_cache_append_paged
decode = fa_mi355x.flash_attention_decode
decode_paged = fa_mi355x.flash_attention_decode_paged


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _i32(vals):
    return torch.tensor(list(vals), dtype=torch.int32, device=DEV)


def _rand_bits(shape, g):
    """Random 16-bit patterns (NaN patterns included: a 16-bit cache takes a bit copy)."""
    return torch.randint(-32768, 32768, shape, generator=g, dtype=torch.int32).to(torch.int16)


def _table(b, cols, g, spare=2):
    """A permuted pool: b * cols table entries into b * cols + spare pages."""
    n = b * cols + spare
    perm = torch.randperm(n, generator=g).to(torch.int32)
    return perm[:b * cols].reshape(b, cols).contiguous(), n


def _expect(cache, src, lens, new_lens=None, table=None):
    """The contract by torch indexing on the CPU.  cache: [B,Hkv,cap,D] or
    (table given) the pool [P,Hkv,page,D]; src: [B,Hkv,Sn,D] of cache's dtype."""
    out = cache.clone()
    sn = src.shape[2]
    for b, ln in enumerate(lens):
        n = sn if new_lens is None else min(max(int(new_lens[b]), 0), sn)
        for t in range(n):
            r = int(ln) - n + t
            if table is None:
                if 0 <= r < cache.shape[2]:
                    out[b, :, r] = src[b, :, t]
            elif 0 <= r < table.shape[1] * cache.shape[2]:
                pid = int(table[b, r // cache.shape[2]])
                if 0 <= pid < cache.shape[0]:
                    out[pid, :, r % cache.shape[2]] = src[b, :, t]
    return out


def _quantise(x, scales):
    """CPU reference bytes of a [B,Hkv,S,D] 16-bit CPU tensor, one scale per head."""
    return torch.stack([torch_reference_bytes(x[:, h], float(scales[h])) for h in range(x.shape[1])], 1)


def _run(k_new, v_new, kc, vc, lens, new_lens=None, table=None, **kw):
    if table is None:
        append(k_new, v_new, kc, vc, lens, new_lens, **kw)
    else:
        append_paged(k_new, v_new, kc, vc, table, lens, new_lens, **kw)
    torch.cuda.synchronize()


def _check_16(dtype, d, paged, hkv, sn, lens, new_lens=None, seed=0):
    g = _gen(seed)
    b = len(lens)
    kn, vn = _rand_bits((b, hkv, sn, d), g), _rand_bits((b, hkv, sn, d), g)
    table = None
    shape = (b, hkv, CAP, d)
    if paged:
        table, npages = _table(b, COLS, g)
        shape = (npages, hkv, PAGE, d)
    k0 = torch.full(shape, SENT16, dtype=torch.int16)
    v0 = torch.full(shape, SENT16 ^ 0x0101, dtype=torch.int16)
    kc, vc = k0.to(DEV).view(dtype), v0.to(DEV).view(dtype)
    _run(kn.to(DEV).view(dtype), vn.to(DEV).view(dtype), kc, vc, _i32(lens),
         None if new_lens is None else _i32(new_lens), None if table is None else table.to(DEV))
    assert torch.equal(kc.view(torch.int16).cpu(), _expect(k0, kn, lens, new_lens, table))
    assert torch.equal(vc.view(torch.int16).cpu(), _expect(v0, vn, lens, new_lens, table))


@pytest.mark.parametrize("sn", [1, 3, 16, 67])
@pytest.mark.parametrize("paged", [False, True], ids=["contig", "paged"])
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("dtype", DTYPES)
def test_append_16bit_whole_cache(dtype, d, paged, sn):
    _check_16(dtype, d, paged, 2, sn, LENS[sn], seed=sn + d)


@pytest.mark.parametrize("paged", [False, True], ids=["contig", "paged"])
def test_append_16bit_one_kv_head(paged):
    _check_16(torch.float16, 128, paged, 1, 16, LENS[16], seed=5)


@pytest.mark.parametrize("paged", [False, True], ids=["contig", "paged"])
@pytest.mark.parametrize("d", [64, 128])
def test_new_lens(d, paged):
    """0, 1, Sn, Sn + 4 (clamped to Sn) and -3 (nothing written) in one batch."""
    sn = 16
    _check_16(torch.bfloat16, d, paged, 2, sn, (40, 66, 70, 192, 100), (0, 1, sn, sn + 4, -3), seed=9)


K_SCALE, V_SCALE = (0.25, 0.3), (3.7, 2.0 ** -6)


def _exhaustive_inputs(dtype):
    """k_new: every bit pattern of the type once ([1, 2, 256, 128]); v_new: the
    same patterns in another order."""
    x = all_patterns(dtype)
    perm = torch.randperm(65536, generator=_gen(3))
    return x.reshape(1, 2, 256, 128), x[perm].reshape(1, 2, 256, 128).contiguous()


def _check_bytes(got, src, scales, what):
    """got: uint8 CPU [1, 2, 256, 128]; bytes equal the CPU reference for every
    non-NaN input, NaN inputs hold a NaN code."""
    want = _quantise(src, scales)
    nan = torch.isnan(src.float())
    assert int(nan.sum()) == NAN_PATTERNS[src.dtype]
    bad = (got != want) & ~nan
    if bool(bad.any()):
        idx = bad.nonzero()[:8].tolist()
        raise AssertionError((what, [(i, hex(int(src.view(torch.int16)[tuple(i)]) & 0xffff),
                                      hex(int(got[tuple(i)])), hex(int(want[tuple(i)]))) for i in idx]))
    assert bool(((got[nan] & 0x7f) == 0x7f).all()), what


@pytest.mark.parametrize("paged", [False, True], ids=["contig", "paged"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_fp8_every_bit_pattern(dtype, paged):
    """All 65536 patterns through K (and, reordered, through V); head 0 and head
    1, K and V each with a scale of their own, a power of two and not.  A kernel
    that uses head 0's scale everywhere or K's scale for V fails."""
    kn, vn = _exhaustive_inputs(dtype)
    g = _gen(4)
    table, npages = (None, 0)
    shape = (1, 2, 256, 128)
    if paged:
        table, npages = _table(1, 4, g)
        shape = (npages, 2, PAGE, 128)
    lens = _i32([256])
    ks, vs = (torch.tensor(s, dtype=torch.float32) for s in (K_SCALE, V_SCALE))

    def run(k_scale, v_scale):
        kc = torch.full(shape, SENT8, dtype=torch.uint8, device=DEV).view(FP8)
        vc = torch.full(shape, SENT8, dtype=torch.uint8, device=DEV).view(FP8)
        _run(kn.to(DEV), vn.to(DEV), kc, vc, lens, None, None if table is None else table.to(DEV),
             k_scale=k_scale, v_scale=v_scale)
        kb, vb = kc.view(torch.uint8).cpu(), vc.view(torch.uint8).cpu()
        if table is not None:  # gather the four pages; the two spare ones keep the sentinel
            used = table[0].long()
            spare = [i for i in range(npages) if i not in used.tolist()]
            assert bool((kb[spare] == SENT8).all()) and bool((vb[spare] == SENT8).all())
            kb, vb = (x[used].permute(1, 0, 2, 3).reshape(1, 2, 256, 128) for x in (kb, vb))
        return kb, vb

    kb, vb = run(ks.to(DEV), vs.to(DEV))
    _check_bytes(kb, kn, ks, "k")
    _check_bytes(vb, vn, vs, "v")
    # NULL scales are scales of 1.0
    ones = torch.ones(2, dtype=torch.float32, device=DEV)
    kb0, vb0 = run(None, None)
    kb1, vb1 = run(ones, ones)
    assert torch.equal(kb0, kb1) and torch.equal(vb0, vb1)
    _check_bytes(kb0, kn, (1.0, 1.0), "k, no scale")


@pytest.mark.parametrize("kv8", [False, True], ids=["16", "kv8"])
def test_out_of_pool_page_ids_write_nothing(kv8):
    """Ids -1 and num_pages in table entries the append uses: the rows mapped
    there are dropped.  The pool is the middle of a larger tensor with one
    sentinel page of slack on each side, which must keep the sentinel."""
    g = _gen(6)
    b, hkv, d, sn = 3, 2, 128, 67
    table, npages = _table(b, COLS, g)
    table[0, 0] = -1
    table[1, 2] = npages
    lens = (67, 192, 130)  # element 0 writes columns 0 and 1, element 1 column 1 and 2
    kn, vn = _rand_bits((b, hkv, sn, d), g).view(torch.float16), _rand_bits((b, hkv, sn, d), g).view(torch.float16)
    if kv8:
        big_k = torch.full((npages + 2, hkv, PAGE, d), SENT8, dtype=torch.uint8)
        # no NaN inputs here: which of the two NaN codes is stored is not specified
        kn, vn = (torch.where(torch.isnan(x.float()), torch.zeros_like(x), x) for x in (kn, vn))
        src_k, src_v = _quantise(kn, (1.0, 1.0)), _quantise(vn, (1.0, 1.0))
        view = lambda x: x.view(FP8)  # noqa: E731
    else:
        big_k = torch.full((npages + 2, hkv, PAGE, d), SENT16, dtype=torch.int16)
        src_k, src_v = kn.view(torch.int16), vn.view(torch.int16)
        view = lambda x: x.view(torch.float16)  # noqa: E731
    big_v = big_k.clone()
    dk, dv = big_k.to(DEV), big_v.to(DEV)
    pk, pv = view(dk)[1:-1], view(dv)[1:-1]
    assert pk.is_contiguous() and pk.data_ptr() != dk.data_ptr()
    _run(kn.to(DEV), vn.to(DEV), pk, pv, _i32(lens), None, table.to(DEV))
    for dev_big, host_big, src in ((dk, big_k, src_k), (dv, big_v, src_v)):
        want = host_big.clone()
        want[1:-1] = _expect(host_big[1:-1], src, lens, None, table)
        got = dev_big.cpu()
        assert torch.equal(got[0], host_big[0]) and torch.equal(got[-1], host_big[-1])
        assert torch.equal(got, want)
    # the dropped rows were really in use: the expectation differs from "all rows written"
    assert not torch.equal(_expect(big_k[1:-1], src_k, lens, None, table.clamp(0, npages - 1)),
                           _expect(big_k[1:-1], src_k, lens, None, table))


def _scatter_to_pool(cache, table, npages):
    """The pool holding `cache` ([B,Hkv,cap,D]) under `table`; other pages zero."""
    b, hkv, cap, d = cache.shape
    pool = torch.zeros((npages, hkv, PAGE, d), dtype=cache.dtype, device=cache.device)
    for i in range(b):
        for j in range(table.shape[1]):
            pool[int(table[i, j])] = cache[i, :, j * PAGE:(j + 1) * PAGE]
    return pool


@pytest.mark.parametrize("ns", [1, 3])
@pytest.mark.parametrize("form", FORMS)
def test_round_trip_append_then_decode(form, ns):
    """Three steps of one token, then one of Sn = 5 with ragged new_lens, into a
    cache whose prefix torch wrote: after each step decode on the appended cache
    equals decode on a cache built wholly by torch (FP8: quantised by the CPU
    reference), O and LSE bit for bit."""
    paged, kv8 = form
    g = _gen(7)
    b, hq, hkv, d = 3, 4, 2, 128
    dtype = torch.float16
    full_k = (torch.randn((b, hkv, CAP, d), generator=g) * 0.5).to(dtype)
    full_v = (torch.randn((b, hkv, CAP, d), generator=g) * 0.5).to(dtype)
    q = (torch.randn((b, hq, 1, d), generator=g)).to(dtype).to(DEV)
    ks, vs = (torch.tensor(s, dtype=torch.float32) for s in ((0.01, 0.0078125), (0.0039, 0.02)))
    scales = dict(k_scale=ks.to(DEV), v_scale=vs.to(DEV)) if kv8 else {}
    table, npages = _table(b, COLS, g)

    def built(full, sc, lens):
        """The cache holding rows [0, len_b) of `full`, zeros elsewhere, by torch alone."""
        c = _quantise(full, sc).view(FP8) if kv8 else full.clone()
        for i, n in enumerate(lens):
            c[i, :, n:].view(torch.uint8 if kv8 else torch.int16).zero_()
        c = c.to(DEV)
        return _scatter_to_pool(c, table, npages) if paged else c

    def dec(kc, vc, lens):
        if paged:
            return decode_paged(q, kc, vc, table.to(DEV), _i32(lens), return_lse=True, num_splits=ns, **scales)
        return decode(q, kc, vc, _i32(lens), return_lse=True, num_splits=ns, **scales)

    lens = [5, 64, 100]
    kc, vc = built(full_k, ks, lens), built(full_v, vs, lens)
    steps = [(1, None)] * 3 + [(5, (5, 2, 0))]
    for sn, new_lens in steps:
        n = [sn] * b if new_lens is None else list(new_lens)
        lens = [a + c for a, c in zip(lens, n)]
        kn = torch.full((b, hkv, sn, d), 77.0, dtype=dtype)  # tokens past n_b: never stored
        vn = kn.clone()
        for i in range(b):
            kn[i, :, :n[i]] = full_k[i, :, lens[i] - n[i]:lens[i]]
            vn[i, :, :n[i]] = full_v[i, :, lens[i] - n[i]:lens[i]]
        _run(kn.to(DEV), vn.to(DEV), kc, vc, _i32(lens), None if new_lens is None else _i32(new_lens),
             table.to(DEV) if paged else None, **scales)
        want_k, want_v = built(full_k, ks, lens), built(full_v, vs, lens)
        raw = torch.uint8 if kv8 else torch.int16
        assert torch.equal(kc.view(raw), want_k.view(raw)) and torch.equal(vc.view(raw), want_v.view(raw))
        o, lse = dec(kc, vc, lens)
        wo, wlse = dec(want_k, want_v, lens)
        torch.cuda.synchronize()
        assert torch.equal(o.view(torch.int16), wo.view(torch.int16)), (sn, lens)
        assert torch.equal(lse.view(torch.int32), wlse.view(torch.int32)), (sn, lens)


@pytest.mark.parametrize("form", FORMS)
def test_graph_capture_append_then_decode(form):
    """Append + decode captured on one stream in one graph; k_new, v_new, kv_lens
    (+1), one table row and the scales are rewritten in place between replays and
    each replay equals the eager pair on a copy of the cache."""
    paged, kv8 = form
    g = _gen(8)
    b, hq, hkv, d, sn = 3, 4, 2, 128, 1
    dtype = torch.bfloat16
    q = torch.randn((b, hq, 1, d), generator=g).to(dtype).to(DEV)
    table_h, npages = _table(b, COLS, g)
    shape = (npages, hkv, PAGE, d) if paged else (b, hkv, CAP, d)
    init = (torch.randn(shape, generator=g) * 0.5).to(dtype)
    kc = init.to(FP8).to(DEV) if kv8 else init.to(DEV)
    vc = kc.clone()
    kn, vn = (torch.zeros((b, hkv, sn, d), dtype=dtype, device=DEV) for _ in range(2))
    lens, table = _i32([10, 63, 130]), table_h.to(DEV)
    ks, vs = (torch.ones(hkv, dtype=torch.float32, device=DEV) for _ in range(2))
    scales = dict(k_scale=ks, v_scale=vs) if kv8 else {}

    def pair(kcache, vcache):
        if paged:
            append_paged(kn, vn, kcache, vcache, table, lens, **scales)
            return decode_paged(q, kcache, vcache, table, lens, num_splits=1, **scales)
        append(kn, vn, kcache, vcache, lens, **scales)
        return decode(q, kcache, vcache, lens, num_splits=1, **scales)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        pair(kc, vc)  # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = pair(kc, vc)
    raw = torch.uint8 if kv8 else torch.int16
    prev = None
    for step in range(3):
        kn.copy_((torch.randn(kn.shape, generator=g) * 0.5).to(dtype))
        vn.copy_((torch.randn(vn.shape, generator=g) * 0.5).to(dtype))
        lens.add_(1)
        if paged:
            table[step % b] = table[step % b].flip(0)
        ks.copy_(torch.tensor([0.5 + step, 0.3], dtype=torch.float32))
        vs.copy_(torch.tensor([0.7, 2.0 ** -step], dtype=torch.float32))
        kcopy, vcopy = kc.clone(), vc.clone()
        want = pair(kcopy, vcopy).clone()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out.view(torch.int16), want.view(torch.int16)), step
        assert torch.equal(kc.view(raw), kcopy.view(raw)) and torch.equal(vc.view(raw), vcopy.view(raw))
        assert prev is None or not torch.equal(prev, want)
        prev = want


@pytest.mark.parametrize("form", FORMS)
def test_torch_ops_equal_python_functions(form):
    import fa_mi355x.torch_op  # noqa: F401

    paged, kv8 = form
    g = _gen(10)
    b, hkv, d, sn = 3, 2, 64, 16
    dtype = torch.float16
    kn, vn = ((torch.randn((b, hkv, sn, d), generator=g) * 4).to(dtype).to(DEV) for _ in range(2))
    table_h, npages = _table(b, COLS, g)
    shape = (npages, hkv, PAGE, d) if paged else (b, hkv, CAP, d)
    cdt, raw = (FP8, torch.uint8) if kv8 else (dtype, torch.int16)
    lens, new_lens, table = _i32(LENS[16]), _i32((16, 3, 0)), table_h.to(DEV)
    sc = [torch.tensor(s, dtype=torch.float32, device=DEV) for s in (K_SCALE, V_SCALE)] if kv8 else [None, None]
    caches = [torch.full(shape, SENT8, dtype=torch.uint8, device=DEV).view(cdt) if kv8 else
              torch.full(shape, SENT16, dtype=torch.int16, device=DEV).view(cdt) for _ in range(4)]
    if paged:
        append_paged(kn, vn, caches[0], caches[1], table, lens, new_lens, *sc)
        ret = torch.ops.fa_mi355x.cache_append_paged(kn, vn, caches[2], caches[3], table, lens, new_lens, *sc)
    else:
        append(kn, vn, caches[0], caches[1], lens, new_lens, *sc)
        ret = torch.ops.fa_mi355x.cache_append(kn, vn, caches[2], caches[3], lens, new_lens, *sc)
    torch.cuda.synchronize()
    assert ret is None
    assert torch.equal(caches[0].view(raw), caches[2].view(raw))
    assert torch.equal(caches[1].view(raw), caches[3].view(raw))
    assert bool((caches[0].view(raw) != (SENT8 if kv8 else SENT16)).any())  # something was written
