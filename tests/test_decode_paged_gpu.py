"""GPU tests of the paged decode-attention entry (fa_decode_paged_f16 /
fa_decode_paged_bf16, fa_mi355x.flash_attention_decode_paged,
torch.ops.fa_mi355x.decode_paged): decode attention over a page pool
[num_pages][Hkv][page_size][D] addressed through a block table.

The acceptance criterion is bit-identity: for the same data and the same
num_splits the paged entry's O and LSE equal (torch.equal) those of the
contiguous entry (fa_mi355x.flash_attention_decode) on the cache gathered from
the pool through the table.  Correctness does not rest on the contiguous
kernel alone: an independent reference is checked at the project's gates
(helpers and gates of tests/decode_refs.py: fp16 vs the CPU oracle 1e-3,
bf16 vs fp32 torch 5e-3, LSE 2^-10 max|score| + 1e-5).

Pools are built by decode_refs.paginate(): a contiguous cache cut into pages,
scattered under a seeded random permutation that interleaves the batch
elements' pages into a pool larger than needed; pages no sequence uses, and the
rows past each length inside the last used page, hold a NaN bit pattern.
"""
import numpy as np
import pytest
import torch

import decode_refs as dr
import fa_mi355x

pytestmark = pytest.mark.gpu

DEV = "cuda"

paged = fa_mi355x.flash_attention_decode_paged
contig = fa_mi355x.flash_attention_decode


def _identity_case(b, hq, hkv, sq, d, dtype, page_size, lens, mpp, splits=(1, 3, 0), seed=3):
    cap = mpp * page_size
    q = dr.rand((b, hq, sq, d), dtype, seed)
    k = dr.rand((b, hkv, cap, d), dtype, seed + 1)
    v = dr.rand((b, hkv, cap, d), dtype, seed + 2)
    kp, vp, table = dr.paginate(k, v, page_size, lens, seed=seed)
    kg, vg = dr.gather(kp, table), dr.gather(vp, table)
    tl = dr.lens(lens)
    for ns in splits:
        got = paged(q, kp, vp, table, tl, causal=True, return_lse=True, num_splits=ns)
        want = contig(q, kg, vg, tl, causal=True, return_lse=True, num_splits=ns)
        assert torch.isfinite(got[0]).all(), (lens, ns)
        assert dr.same(got, want), (b, hq, hkv, sq, d, dtype, page_size, tuple(lens), ns)


# ---- 1. bit-identity with the contiguous entry -------------------------------------

@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("d", [128, 64])
@pytest.mark.parametrize("page_size", [64, 128, 192])
def test_bit_identical_to_contiguous(page_size, d, dtype):
    ps = page_size
    # a ragged batch: an empty element, one key into the second page, one short of three pages
    _identity_case(3, 8, 2, 1, d, dtype, ps, (0, ps + 1, 3 * ps - 1), mpp=3)
    # one element: fewer tiles than waves, tile and page edges, a full table row
    for n in sorted({1, 63, 64, 65, ps - 1, ps, ps + 1, 4 * ps}):
        _identity_case(1, 8, 2, 1, d, dtype, ps, (n,), mpp=4, seed=n)


@pytest.mark.parametrize("d", [128, 64])
@pytest.mark.parametrize("g,sq", [(1, 1), (4, 4), (7, 3), (16, 4), (16, 5)])
def test_bit_identical_row_blocks(g, sq, d):
    """1 / 2 / 4 row blocks; (16, 4) at head_dim 128 parks Q in LDS, (16, 5)
    has a second row group."""
    for dtype in (torch.float16, torch.bfloat16):
        _identity_case(1, 2 * g, 2, sq, d, dtype, 128, (300,), mpp=3)


# ---- 2. independent reference ---------------------------------------------------

_REFS = {}


def _ref_f16(sq, causal):
    """Inputs (uint16 bits, cap 1152 = 18 pages of 64 = 6 of 192) and the CPU
    oracle's O / float64 LSE for lens (300, 1000); computed once, read-only."""
    key = (sq, causal)
    if key not in _REFS:
        q, k, v = dr.inputs(2, 8, 2, sq, 1152, 128)
        lens = np.array([300, 1000])
        _REFS[key] = (q, k, v, lens, dr.oracle_decode(q, k, v, lens, causal),
                      dr.lse_ref(q, k, v, lens, causal))
    return _REFS[key]


@pytest.mark.parametrize("sq", [1, 5])
@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("page_size", [64, 192])
def test_against_references(page_size, causal, sq):
    q, k, v, lens, ref, (lref, smax) = _ref_f16(sq, causal)
    tq, tk, tv, tl = dr.dev(q), dr.dev(k), dr.dev(v), dr.lens(lens)
    kp, vp, table = dr.paginate(tk, tv, page_size, lens, seed=11)
    what = f"paged ps={page_size} causal={causal} Sq={sq}"
    out, lse = paged(tq, kp, vp, table, tl, causal=causal, return_lse=True)
    dr.check_f16(out, ref, "fp16 " + what)
    dr.check_lse(lse, lref, smax, "fp16 " + what)
    # bf16 against fp32 torch on the gathered cache
    bq, bk, bv = (t.to(torch.bfloat16) for t in (tq, tk, tv))
    kp, vp, table = dr.paginate(bk, bv, page_size, lens, seed=12)
    out, lse = paged(bq, kp, vp, table, tl, causal=causal, return_lse=True)
    ro, _ = dr.ref_torch(bq, dr.gather(kp, table), dr.gather(vp, table), tl, causal)
    err = float((out.float() - ro).abs().max())
    print(f"bf16 {what}: {err:.3e}")
    assert err <= dr.GATE_BF16, (what, err)
    bref, bsmax = dr.lse_ref(bq, bk, bv, lens, causal)
    dr.check_lse(lse, bref, bsmax, "bf16 " + what)


def test_one_key_and_unseen_rows():
    q, k, v = dr.inputs(1, 8, 2, 5, 128, 128)
    tq, tk, tv = dr.dev(q), dr.dev(k), dr.dev(v)
    # one key: P = 1, O is that V row exactly
    kp, vp, table = dr.paginate(tk, tv, 64, (1,), seed=1)
    out = paged(tq[:, :, :1].contiguous(), kp, vp, table, dr.lens([1]), causal=True)
    got = dr.bits(out)
    for h in range(8):
        assert np.array_equal(got[0, h, 0], v[0, h // 4, 0]), h
    # three keys, five causal query tokens: the first two see no key
    kp, vp, table = dr.paginate(tk, tv, 64, (3,), seed=2)
    out, lse = paged(tq, kp, vp, table, dr.lens([3]), causal=True, return_lse=True)
    assert int(torch.count_nonzero(out[:, :, :2])) == 0
    assert torch.isneginf(lse[:, :, :2]).all() and torch.isfinite(lse[:, :, 2:]).all()
    dr.check_f16(out, dr.oracle_decode(q, k, v, np.array([3]), True), "three keys, Sq=5")


# ---- 3. padding and unused entries ------------------------------------------------

@pytest.mark.parametrize("splits", [1, 3])
def test_nan_padding_and_junk_entries(splits):
    """Unused pages and the rows past each length are NaN; table entries past
    each length are arbitrary ids (out-of-pool ones among them): never read."""
    lens = (0, 129, 700, 1)
    q = dr.rand((4, 8, 2, 128), torch.float16, 20)
    k = dr.rand((4, 2, 768, 128), torch.float16, 21)
    v = dr.rand((4, 2, 768, 128), torch.float16, 22)
    tl = dr.lens(lens)
    kp, vp, zeros = dr.paginate(k, v, 128, lens, seed=5, filler=0)
    kp2, vp2, junk = dr.paginate(k, v, 128, lens, seed=5, filler="junk")
    assert torch.equal(kp.view(torch.int16), kp2.view(torch.int16)) and not torch.equal(zeros, junk)
    want = paged(q, kp, vp, zeros, tl, causal=True, return_lse=True, num_splits=splits)
    got = paged(q, kp, vp, junk, tl, causal=True, return_lse=True, num_splits=splits)
    assert torch.isfinite(got[0]).all()
    assert dr.same(got, want)


# ---- 4. out-of-range ids ----------------------------------------------------------

@pytest.mark.parametrize("splits", [1, 3])
def test_out_of_range_page_ids(splits):
    """Ids -2, -1, num_pages, num_pages + 1 in entries that ARE read.  The pool
    is a slice of a larger NaN-filled allocation, two pages in from either end,
    so even a missing clamp reads only this test's memory -- and then NaN."""
    lens = (200, 300, 129)
    q = dr.rand((3, 8, 1, 128), torch.float16, 30)
    k = dr.rand((3, 2, 320, 128), torch.float16, 31)
    v = dr.rand((3, 2, 320, 128), torch.float16, 32)
    tl = dr.lens(lens)
    kp0, vp0, table = dr.paginate(k, v, 64, lens, seed=6)
    n = kp0.shape[0]
    bigk = dr.nan_fill(torch.empty((n + 4,) + tuple(kp0.shape[1:]), dtype=kp0.dtype, device=DEV))
    bigv = dr.nan_fill(torch.empty_like(bigk))
    kp, vp = bigk[2:2 + n], bigv[2:2 + n]
    kp.copy_(kp0)
    vp.copy_(vp0)
    assert kp.is_contiguous() and vp.is_contiguous()
    want = paged(q, kp, vp, table, tl, causal=True, return_lse=True, num_splits=splits)
    bad = table.clone()
    bad[1, 0], bad[1, 1], bad[1, 3], bad[1, 4] = -2, -1, n, n + 1  # element 1 reads entries 0..4
    got = paged(q, kp, vp, bad, tl, causal=True, return_lse=True, num_splits=splits)
    for bi in (0, 2):
        assert torch.equal(got[0][bi], want[0][bi]) and torch.equal(got[1][bi], want[1][bi]), bi
    assert torch.isfinite(got[0][1]).all()
    assert not torch.isnan(got[1][1]).any()


# ---- 5. sharing and repeats -------------------------------------------------------

def test_shared_and_repeated_pages():
    q = dr.rand((2, 8, 2, 128), torch.float16, 40)
    q[1] = q[0]
    k = dr.rand((1, 2, 512, 128), torch.float16, 41)
    v = dr.rand((1, 2, 512, 128), torch.float16, 42)
    kp, vp, table = dr.paginate(k, v, 128, (500,), seed=7)
    # two elements naming the same pages, same length: equal outputs
    both = table.repeat(2, 1).contiguous()
    out, lse = paged(q, kp, vp, both, dr.lens([500, 500]), causal=True, return_lse=True)
    assert torch.equal(out[0], out[1]) and torch.equal(lse[0], lse[1])
    one = paged(q[:1].contiguous(), kp, vp, table, dr.lens([500]), causal=True)
    assert torch.equal(out[:1], one)
    # one page listed twice: the contiguous run on the cache with those rows repeated
    rep = table[:, [0, 1, 1, 2]].contiguous()
    tl = dr.lens([512])
    got = paged(q[:1].contiguous(), kp, vp, rep, tl, causal=True, return_lse=True, num_splits=2)
    want = contig(q[:1].contiguous(), dr.gather(kp, rep), dr.gather(vp, rep), tl, causal=True,
                  return_lse=True, num_splits=2)
    assert dr.same(got, want)


# ---- 6. permutation invariance ----------------------------------------------------

def test_placement_does_not_matter():
    lens = (700, 65, 384)
    q = dr.rand((3, 8, 1, 64), torch.bfloat16, 50)
    k = dr.rand((3, 2, 768, 64), torch.bfloat16, 51)
    v = dr.rand((3, 2, 768, 64), torch.bfloat16, 52)
    tl = dr.lens(lens)
    a = dr.paginate(k, v, 192, lens, seed=8)
    b = dr.paginate(k, v, 192, lens, seed=9, spare=11)
    assert not torch.equal(a[2], b[2])
    for ns in (0, 2):
        assert dr.same(paged(q, *a, tl, causal=True, return_lse=True, num_splits=ns),
                     paged(q, *b, tl, causal=True, return_lse=True, num_splits=ns))


# ---- 7. 64-bit page offsets -------------------------------------------------------

def test_pool_past_4gib():
    """A pool of more than 4 GiB: a 32-bit page offset would read another page."""
    npages, hkv, ps, d = 8200, 8, 256, 128
    assert npages * hkv * ps * d * 2 > 4 << 30
    try:
        kp = torch.empty((npages, hkv, ps, d), dtype=torch.float16, device=DEV)
        vp = torch.empty_like(kp)
    except RuntimeError as e:  # torch.cuda.OutOfMemoryError is one
        pytest.skip(f"cannot allocate two pools of {npages * hkv * ps * d * 2 >> 20} MiB: {e}")
    n = 4 * ps - 3
    q = dr.rand((1, hkv, 1, d), torch.float16, 60)
    k = dr.rand((1, hkv, 4 * ps, d), torch.float16, 61)
    v = dr.rand((1, hkv, 4 * ps, d), torch.float16, 62)
    ids = [npages - 2, npages - 4, npages - 1, npages - 3]  # the top of the pool
    for j, pg in enumerate(ids):
        kp[pg] = k[0, :, j * ps:(j + 1) * ps]
        vp[pg] = v[0, :, j * ps:(j + 1) * ps]
    table = torch.tensor([ids], dtype=torch.int32, device=DEV)
    tl = dr.lens([n])
    out = paged(q, kp, vp, table, tl, causal=True)
    ro, _ = dr.ref_torch(q, k, v, tl, True)
    err = float((out.float() - ro).abs().max())
    print(f"4 GiB pool: {err:.3e}")
    del kp, vp
    torch.cuda.empty_cache()
    assert err <= dr.GATE_F16


# ---- 8. workspace -----------------------------------------------------------------

def test_forced_splits_workspace():
    q, k, v = (dr.dev(a) for a in dr.inputs(1, 8, 2, 1, 1024, 128))
    lens = (1000,)
    tl = dr.lens(lens)
    kp, vp, table = dr.paginate(k, v, 64, lens, seed=13)
    dev = torch.cuda.current_device()
    st = torch.cuda.current_stream().cuda_stream
    for ns in (2, 7, 16):
        out = paged(q, kp, vp, table, tl, causal=True, num_splits=ns)
        assert dr.ws_counters_zero(), ns
        assert torch.equal(out, contig(q, k, v, tl, causal=True, num_splits=ns)), ns
        again = paged(q, kp, vp, table, tl, causal=True, num_splits=ns)
        assert torch.equal(out, again), ns
        assert dr.ws_counters_zero(), ns
        # poison the slabs: every slab the merge reads was written by this launch
        fa_mi355x._WS_BUF[(dev, st)][65536:].fill_(0xff)
        poisoned = paged(q, kp, vp, table, tl, causal=True, num_splits=ns)
        assert torch.equal(out, poisoned), ns
        assert dr.ws_counters_zero(), ns


def test_workspace_shared_with_forward_and_contiguous():
    """One per-stream workspace serves paged decode, forward and contiguous
    decode launches in any order."""
    import oracle

    q, k, v = dr.inputs(1, 8, 2, 1, 1024, 128)
    tq, tk, tv = dr.dev(q), dr.dev(k), dr.dev(v)
    lens = np.array([1000])
    tl = dr.lens(lens)
    ref = dr.oracle_decode(q, k, v, lens, True)
    kp, vp, table = dr.paginate(tk, tv, 64, lens, seed=14)
    fq, fk, fv = oracle.gen_inputs(1, 4, 8192, 128, 7)
    assert fa_mi355x.workspace_bytes(1, 4, 8192, 128, True) > 65536  # the split tier
    rows = np.array([0, 255, 4096, 8191])
    fref = oracle.attention_rows(fq[0, 3], fk[0, 3], fv[0, 3], rows, True)

    p1 = paged(tq, kp, vp, table, tl, causal=True, num_splits=4)
    fo = fa_mi355x.flash_attention_fwd(dr.dev(fq), dr.dev(fk), dr.dev(fv), causal=True)
    c1 = contig(tq, tk, tv, tl, causal=True, num_splits=4)
    p2 = paged(tq, kp, vp, table, tl, causal=True, num_splits=4)
    assert dr.ws_counters_zero()
    dr.check_f16(p1, ref, "paged decode before forward")
    dr.check_f16(fo[0, 3, rows], fref, "forward between decodes")
    assert torch.equal(p1, c1) and torch.equal(p1, p2)


# ---- 9. entry points --------------------------------------------------------------

def test_torch_op_matches_python_entry():
    import fa_mi355x.torch_op  # noqa: F401

    q, k, v = (dr.dev(a) for a in dr.inputs(2, 8, 2, 2, 640, 128))
    lens = (77, 600)
    tl = dr.lens(lens)
    kp, vp, table = dr.paginate(k, v, 128, lens, seed=15)
    want = paged(q, kp, vp, table, tl, causal=True)
    assert torch.equal(torch.ops.fa_mi355x.decode_paged(q, kp, vp, table, tl, True), want)
    # no kv_lens: every length is the table's capacity
    kp2, vp2, table2 = dr.paginate(k, v, 128, (640, 640), seed=16)
    assert torch.equal(torch.ops.fa_mi355x.decode_paged(q, kp2, vp2, table2),
                       paged(q, kp2, vp2, table2))

    def f(q, kp, vp, table, lens):
        return torch.ops.fa_mi355x.decode_paged(q, kp, vp, table, lens, causal=True) + 0

    with torch.no_grad():
        comp = torch.compile(f, backend="eager", fullgraph=True)(q, kp, vp, table, tl)
    assert torch.equal(comp, want)


def test_wrapper_rejections_on_device():
    """The wrapper's rejections with real device tensors: each names its cause
    and nothing is launched (an int64 table would otherwise be read as int32)."""
    import fa_mi355x.torch_op  # noqa: F401

    q, k, v = (dr.dev(a) for a in dr.inputs(2, 8, 2, 1, 640, 128))
    kp, vp, table = dr.paginate(k, v, 128, (600, 5), seed=17)
    err = fa_mi355x.FlashAttentionError
    with pytest.raises(err, match="block_table must be a tensor on"):
        paged(q, kp, vp, table.cpu())
    with pytest.raises(err, match="block_table must be int32"):
        paged(q, kp, vp, table.long())
    with pytest.raises(err, match="block_table has 3 rows, q a batch of 2"):
        paged(q, kp, vp, torch.cat([table, table[:1]]).contiguous())
    with pytest.raises(err, match="block_table must be contiguous"):
        paged(q, kp, vp, table.t().contiguous().t())
    with pytest.raises(err, match="kv_lens must be a tensor on"):
        paged(q, kp, vp, table, torch.tensor([5, 600], dtype=torch.int32))
    with pytest.raises(err, match="k_pages must be a device tensor"):
        paged(q, kp.cpu(), vp, table)
    # a strided view of a larger pool is refused, by the op too: no hidden copy of the pool
    with pytest.raises(err, match="k_pages must be contiguous"):
        paged(q, kp[:, :, :64], vp[:, :, :64], table)
    with pytest.raises(err, match="k_pages must be contiguous"):
        torch.ops.fa_mi355x.decode_paged(q, kp[:, :, :64], vp[:, :, :64], table)


# ---- 10. graph replay -------------------------------------------------------------

def test_op_in_hip_graph_follows_lengths_and_table():
    """One linear capture, one replay; between them kv_lens changes and the
    block table is rewritten in place to another placement of the same data."""
    import fa_mi355x.torch_op  # noqa: F401

    op = torch.ops.fa_mi355x.decode_paged
    q, k, v = (dr.dev(a) for a in dr.inputs(1, 8, 2, 1, 2048, 128))
    kp, vp, table_a = dr.paginate(k, v, 128, (2048,), seed=18, spare=16)
    # the same pages once more, at the places the first placement left free
    free = sorted(set(range(kp.shape[0])) - set(table_a[0].tolist()))
    table_b = torch.tensor([free], dtype=torch.int32, device=DEV)
    kp[table_b[0].long()] = kp[table_a[0].long()]
    vp[table_b[0].long()] = vp[table_a[0].long()]
    assert not (set(table_a[0].tolist()) & set(table_b[0].tolist()))
    table = table_a.clone()
    lens = dr.lens([2048])
    for n in (2048, 700):  # eager references (and the first-launch set-up) outside the capture
        lens.fill_(n)
        op(q, kp, vp, table, lens, True)
    want = op(q, kp, vp, table_b, lens, True).clone()  # lens = 700, the second placement
    assert torch.equal(want, op(q, kp, vp, table_a, lens, True))
    lens.fill_(2048)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        op(q, kp, vp, table, lens, True)  # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = op(q, kp, vp, table, lens, True)
    lens.fill_(700)
    table.copy_(table_b)
    kp[table_a[0].long()] = float("nan")  # the first placement's pages are gone
    vp[table_a[0].long()] = float("nan")
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, want)
