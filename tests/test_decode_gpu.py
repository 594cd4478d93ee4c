"""GPU tests of the decode-attention entry (fa_decode_f16 / fa_decode_bf16,
fa_mi355x.flash_attention_decode, torch.ops.fa_mi355x.decode): a few query
tokens per head over a K/V cache with per-batch lengths, grouped K/V heads and
the in-launch split of the key range.

The references and gates are those of tests/decode_refs.py: fp16 output
against the CPU oracle at 1e-3, bf16 output against fp32 torch at 5e-3, LSE
against a float64 reference at 2^-10 * max|scaled score| + 1e-5.
"""
import numpy as np
import pytest
import torch

import decode_refs as dr
import fa_mi355x
import oracle

pytestmark = pytest.mark.gpu

DEV = "cuda"


# ---- wave and tile edges --------------------------------------------------------

EDGE_LENS = (1, 2, 63, 64, 65, 255, 256, 257, 300)


@pytest.mark.parametrize("n", EDGE_LENS)
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("d", [128, 64])
def test_tile_edges(d, causal, n):
    """Fewer tiles than waves, the ragged last tile, one full wave round +-1
    (B = 1, one head, one query token; the cache's capacity is 300 rows)."""
    q, k, v = dr.inputs(1, 1, 1, 1, 300, d)
    lens = np.array([n])
    out, lse = fa_mi355x.flash_attention_decode(dr.dev(q), dr.dev(k), dr.dev(v), dr.lens(lens),
                                                causal=causal, return_lse=True)
    dr.check_f16(out, dr.oracle_decode(q, k, v, lens, causal), f"edges d={d} causal={causal} len={n}")
    ref, smax = dr.lse_ref(q, k, v, lens, causal)
    dr.check_lse(lse, ref, smax, f"edges d={d} causal={causal} len={n}")
    if n == 1:  # one key: P = 1, O is V[0] exactly
        assert np.array_equal(dr.bits(out)[0, 0, 0], v[0, 0, 0])


# ---- groups ---------------------------------------------------------------------

GROUPS = [(1, 1), (2, 1), (4, 1), (5, 1), (7, 1), (8, 1), (16, 1),
          (4, 4), (7, 3), (8, 8), (16, 5), (1, 16)]


@pytest.mark.parametrize("g,sq", GROUPS)
def test_groups(g, sq):
    """1..80 query rows per K/V head: padded rows, 1 / 2 / 4 row blocks, a second
    row group; a query head's output depends on K/V head h // G only."""
    b, hkv, cap = 2, 2, 1000
    lens = np.array([300, 1000])
    q, k, v = dr.inputs(b, hkv * g, hkv, sq, cap, 128)
    tq, tk, tv, tl = dr.dev(q), dr.dev(k), dr.dev(v), dr.lens(lens)
    out, lse = fa_mi355x.flash_attention_decode(tq, tk, tv, tl, causal=True, return_lse=True)
    dr.check_f16(out, dr.oracle_decode(q, k, v, lens, True), f"groups G={g} Sq={sq}")
    ref, smax = dr.lse_ref(q, k, v, lens, True)
    dr.check_lse(lse, ref, smax, f"groups G={g} Sq={sq}")
    # swap the K/V heads (and the query heads with them): outputs swap
    perm = [1, 0]
    q2 = tq.view(b, hkv, g, sq, 128)[:, perm].reshape(tq.shape).contiguous()
    out2 = fa_mi355x.flash_attention_decode(q2, tk[:, perm].contiguous(), tv[:, perm].contiguous(),
                                            tl, causal=True)
    want = out.view(b, hkv, g, sq, 128)[:, perm].reshape(out.shape)
    assert torch.equal(out2, want)


@pytest.mark.parametrize("g,sq,d", [(4, 4, 128), (7, 3, 64), (16, 5, 128)])
def test_groups_bf16(g, sq, d):
    b, hkv, cap = 2, 2, 1000
    lens = dr.lens([300, 1000])
    q, k, v = (dr.dev(a).to(torch.bfloat16) for a in dr.inputs(b, hkv * g, hkv, sq, cap, d))
    out, lse = fa_mi355x.flash_attention_decode(q, k, v, lens, causal=True, return_lse=True)
    ro, rl = dr.ref_torch(q, k, v, lens, True)
    err = float((out.float() - ro).abs().max())
    print(f"bf16 G={g} Sq={sq} d={d}: max err {err:.3e}")
    assert err <= dr.GATE_BF16
    del rl
    ref, smax = dr.lse_ref(q, k, v, [300, 1000], True)  # float64, of the bf16 inputs
    dr.check_lse(lse, ref, smax, f"bf16 G={g} Sq={sq} d={d}")


# ---- causal with Sq > 1 ---------------------------------------------------------

CAUSAL_ROWS = [(sq, n) for sq in (2, 5, 16) for n in (sq, sq + 1, 64, 65, 200)]


@pytest.mark.parametrize("sq,n", CAUSAL_ROWS)
def test_causal_rows(sq, n):
    """Row t against the oracle row at position len - Sq + t (B = 1)."""
    lens = np.array([n])
    q, k, v = dr.inputs(1, 2, 1, sq, 200, 128)
    out, lse = fa_mi355x.flash_attention_decode(dr.dev(q), dr.dev(k), dr.dev(v), dr.lens(lens),
                                                causal=True, return_lse=True)
    dr.check_f16(out, dr.oracle_decode(q, k, v, lens, True), f"causal Sq={sq} len={n}")
    ref, smax = dr.lse_ref(q, k, v, lens, True)
    dr.check_lse(lse, ref, smax, f"causal Sq={sq} len={n}")


def test_causal_short_cache():
    """kv_lens = 3 with Sq = 5: the first two rows see no key."""
    lens = np.array([3])
    q, k, v = dr.inputs(1, 2, 1, 5, 64, 128)
    out, lse = fa_mi355x.flash_attention_decode(dr.dev(q), dr.dev(k), dr.dev(v), dr.lens(lens),
                                                causal=True, return_lse=True)
    assert int(torch.count_nonzero(out[:, :, :2]).item()) == 0
    assert bool(torch.isneginf(lse[:, :, :2]).all())
    dr.check_f16(out, dr.oracle_decode(q, k, v, lens, True), "short cache")
    ref, smax = dr.lse_ref(q, k, v, lens, True)
    dr.check_lse(lse, ref, smax, "short cache")


# ---- ragged batch ---------------------------------------------------------------

@pytest.mark.parametrize("splits", [1, 3])
def test_ragged_batch_nan_padding(splits):
    lens = np.array([0, 1, 64, 65, 777, 1100])
    b, hq, hkv, cap = 6, 8, 2, 1100
    q, k, v = dr.inputs(b, hq, hkv, 1, cap, 128)
    k, v = k.copy(), v.copy()
    for i, n in enumerate(lens):  # capacity padding: NaN bit patterns
        k[i, :, n:] = 0x7e00
        v[i, :, n:] = 0xfe01
    tq, tk, tv = dr.dev(q), dr.dev(k), dr.dev(v)
    out, lse = fa_mi355x.flash_attention_decode(tq, tk, tv, dr.lens(lens), causal=True,
                                                return_lse=True, num_splits=splits)
    assert bool(torch.isfinite(out).all())
    dr.check_f16(out, dr.oracle_decode(q, k, v, lens, True), f"ragged splits={splits}")
    ref, smax = dr.lse_ref(q, k, v, lens, True)
    dr.check_lse(lse, ref, smax, f"ragged splits={splits}")
    assert int(torch.count_nonzero(out[0]).item()) == 0
    # caches truncated to a common length, no kv_lens: the same bits
    for n in (65, 777):
        explicit = fa_mi355x.flash_attention_decode(tq, tk, tv, dr.lens([n] * b), causal=True,
                                                    num_splits=splits)
        trunc = fa_mi355x.flash_attention_decode(tq, tk[:, :, :n].contiguous(),
                                                 tv[:, :, :n].contiguous(), None, causal=True,
                                                 num_splits=splits)
        sel = [i for i in range(b) if lens[i] >= n]  # elements whose first n rows are all real
        assert torch.equal(explicit[sel], trunc[sel])


# ---- splits ---------------------------------------------------------------------

def test_forced_splits():
    b, hq, hkv, n = 1, 8, 2, 1000
    q, k, v = dr.inputs(b, hq, hkv, 1, n, 128)
    tq, tk, tv = dr.dev(q), dr.dev(k), dr.dev(v)
    lens = np.array([n])
    ref = dr.oracle_decode(q, k, v, lens, True)
    lref, smax = dr.lse_ref(q, k, v, lens, True)
    base = fa_mi355x.flash_attention_decode(tq, tk, tv, causal=True, num_splits=1)
    dr.check_f16(base, ref, "splits=1")
    dev = torch.cuda.current_device()
    st = torch.cuda.current_stream().cuda_stream
    # len 1000 is 16 tiles: 16 pieces have one tile each (three waves idle), 32 pieces
    # leave every other piece without a tile (it hands (-inf, 0) to the merge)
    for ns in (2, 3, 7, 16, 32):
        out, lse = fa_mi355x.flash_attention_decode(tq, tk, tv, causal=True, num_splits=ns,
                                                    return_lse=True)
        assert dr.ws_counters_zero(), ns
        dr.check_f16(out, ref, f"splits={ns}")
        dr.check_lse(lse, lref, smax, f"splits={ns}")
        diff = float((out.float() - base.float()).abs().max())
        print(f"splits={ns}: vs one piece {diff:.3e}")
        assert diff <= 2e-4, (ns, diff)
        again = fa_mi355x.flash_attention_decode(tq, tk, tv, causal=True, num_splits=ns)
        assert torch.equal(out, again), ns
        assert dr.ws_counters_zero(), ns
        # poison the slabs: every slab the merge reads was written by this launch
        fa_mi355x._WS_BUF[(dev, st)][65536:].fill_(0xff)
        poisoned = fa_mi355x.flash_attention_decode(tq, tk, tv, causal=True, num_splits=ns)
        assert torch.equal(out, poisoned), ns
        assert dr.ws_counters_zero(), ns


def test_workspace_shared_with_forward():
    """One per-stream workspace serves decode and forward launches in any order."""
    q, k, v = dr.inputs(1, 8, 2, 1, 1000, 128)
    tq, tk, tv = dr.dev(q), dr.dev(k), dr.dev(v)
    ref = dr.oracle_decode(q, k, v, np.array([1000]), True)
    fq, fk, fv = oracle.gen_inputs(1, 4, 8192, 128, 7)
    assert fa_mi355x.workspace_bytes(1, 4, 8192, 128, True) > 65536  # the split tier
    rows = np.array([0, 255, 4096, 8191])
    fref = oracle.attention_rows(fq[0, 3], fk[0, 3], fv[0, 3], rows, True)
    sq_, sk_, sv_ = dr.inputs(1, 4, 2, 2, 520, 64)
    sref = dr.oracle_decode(sq_, sk_, sv_, np.array([520]), True)

    d1 = fa_mi355x.flash_attention_decode(tq, tk, tv, causal=True, num_splits=4)
    fo = fa_mi355x.flash_attention_fwd(dr.dev(fq), dr.dev(fk), dr.dev(fv), causal=True)
    d2 = fa_mi355x.flash_attention_decode(tq, tk, tv, causal=True, num_splits=4)
    d3 = fa_mi355x.flash_attention_decode(dr.dev(sq_), dr.dev(sk_), dr.dev(sv_), causal=True, num_splits=2)
    assert dr.ws_counters_zero()
    dr.check_f16(d1, ref, "decode before forward")
    assert torch.equal(d1, d2)
    dr.check_f16(fo[0, 3, rows], fref, "forward between decodes")
    dr.check_f16(d3, sref, "smaller decode")


# ---- peaked softmax -------------------------------------------------------------

@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_peaked_softmax(dtype):
    """q and k scaled by 3: the in-wave rescale, the in-CU merge and the
    cross-piece merge all see very different maxima."""
    q, k, v = dr.inputs(1, 8, 2, 1, 1000, 128)
    tq, tk, tv = (dr.dev(a) for a in (q, k, v))
    tq, tk = tq * 3, tk * 3
    if dtype is torch.bfloat16:
        tq, tk, tv = (t.to(dtype) for t in (tq, tk, tv))
        out = fa_mi355x.flash_attention_decode(tq, tk, tv, causal=True, num_splits=4)
        ro, _ = dr.ref_torch(tq, tk, tv, dr.lens([1000]), True)
        err = float((out.float() - ro).abs().max())
        print(f"peaked bf16: {err:.3e}")
        assert err <= dr.GATE_BF16
        return
    out = fa_mi355x.flash_attention_decode(tq, tk, tv, causal=True, num_splits=4)
    ref = dr.oracle_decode(dr.bits(tq), dr.bits(tk), v, np.array([1000]), True)
    dr.check_f16(out, ref, "peaked fp16")


# ---- agreement with the forward path -------------------------------------------

def test_agrees_with_forward():
    q, k, v = oracle.gen_inputs(1, 4, 300, 128, 11)
    tq, tk, tv = dr.dev(q), dr.dev(k), dr.dev(v)
    fwd = fa_mi355x.flash_attention_fwd(tq, tk, tv, causal=True)[:, :, -8:]
    dec = fa_mi355x.flash_attention_decode(tq[:, :, -8:].contiguous(), tk, tv, causal=True)
    assert float((fwd.float() - dec.float()).abs().max()) <= 2e-3
    ref = np.stack([oracle.attention_rows(q[0, h], k[0, h], v[0, h], np.arange(292, 300), True)
                    for h in range(4)])[None]
    dr.check_f16(fwd, ref, "forward, last 8 rows")
    dr.check_f16(dec, ref, "decode, last 8 rows")


# ---- long and large -------------------------------------------------------------

def test_long_cache():
    n = 131072 + 17
    q, k, v = dr.inputs(1, 8, 1, 1, n, 128)
    out, lse = fa_mi355x.flash_attention_decode(dr.dev(q), dr.dev(k), dr.dev(v), causal=True,
                                                return_lse=True)
    dr.check_f16(out, dr.oracle_decode(q, k, v, np.array([n]), True), "long cache")
    ref, smax = dr.lse_ref(q, k, v, np.array([n]), True)
    dr.check_lse(lse, ref, smax, "long cache")


def test_cache_past_4gib():
    """A K cache of more than 4 GiB in one launch: a 32-bit head offset would
    read the wrong head for the last batch element's last K/V head."""
    b, h, cap, d = 16, 8, 131072 + 8, 128
    assert b * h * cap * d * 2 > 4 << 30
    gen = torch.Generator(device=DEV).manual_seed(5)
    k = torch.empty((b, h, cap, d), dtype=torch.float16, device=DEV)
    v = torch.empty_like(k)
    for t in (k, v):
        for i in range(b):  # fp16 uniform [-1, 1), filled on the device
            t[i] = torch.rand((h, cap, d), generator=gen, device=DEV, dtype=torch.float16) * 2 - 1
    q = torch.rand((b, h, 1, d), generator=gen, device=DEV, dtype=torch.float16) * 2 - 1
    out = fa_mi355x.flash_attention_decode(q, k, v, causal=True)
    ro, _ = dr.ref_torch(q[-1:, -1:], k[-1:, -1:], v[-1:, -1:], dr.lens([cap]), True)
    err = float((out[-1:, -1:].float() - ro).abs().max())
    print(f"4 GiB cache: {err:.3e}")
    assert err <= dr.GATE_F16
    del k, v
    torch.cuda.empty_cache()


# ---- entry points ---------------------------------------------------------------

def test_wrapper_rejections_on_device():
    """The wrapper's rejections with real device tensors: each names its cause,
    and nothing is launched (an int64 kv_lens would otherwise be read as int32)."""
    import fa_mi355x.torch_op  # noqa: F401

    q, k, v = (dr.dev(a) for a in dr.inputs(2, 8, 2, 1, 600, 128))
    err = fa_mi355x.FlashAttentionError
    with pytest.raises(err, match="kv_lens must be int32"):
        fa_mi355x.flash_attention_decode(q, k, v, torch.tensor([5, 600], device=DEV))
    with pytest.raises(err, match="kv_lens must be a tensor on"):
        fa_mi355x.flash_attention_decode(q, k, v, torch.tensor([5, 600], dtype=torch.int32))
    with pytest.raises(err, match="kv_lens must be a contiguous"):
        fa_mi355x.flash_attention_decode(q, k, v, dr.lens([5, 600, 7]))
    with pytest.raises(err, match="must have one shape"):
        fa_mi355x.flash_attention_decode(q, k, v[:, :, :500].contiguous())
    with pytest.raises(err, match="not a multiple of heads_kv"):
        fa_mi355x.flash_attention_decode(q[:, :7].contiguous(), k, v)
    with pytest.raises(err, match="q must be float16 or bfloat16"):
        fa_mi355x.flash_attention_decode(q.float(), k.float(), v.float())
    with pytest.raises(err, match="k_cache must be a device tensor"):
        fa_mi355x.flash_attention_decode(q, k.cpu(), v)
    # a strided view of a larger cache is refused, by the op too: no hidden copy of the cache
    with pytest.raises(err, match="k_cache must be contiguous"):
        fa_mi355x.flash_attention_decode(q, k[:, :, :300], v[:, :, :300])
    with pytest.raises(err, match="k_cache must be contiguous"):
        torch.ops.fa_mi355x.decode(q, k[:, :, :300], v[:, :, :300])


def test_torch_op_matches_python_entry():
    import fa_mi355x.torch_op  # noqa: F401

    q, k, v = (dr.dev(a) for a in dr.inputs(2, 8, 2, 2, 600, 128))
    lens = dr.lens([77, 600])
    want = fa_mi355x.flash_attention_decode(q, k, v, lens, causal=True)
    got = torch.ops.fa_mi355x.decode(q, k, v, lens, True)
    assert torch.equal(got, want)
    assert torch.equal(torch.ops.fa_mi355x.decode(q, k, v), fa_mi355x.flash_attention_decode(q, k, v))

    def f(q, k, v, lens):
        return torch.ops.fa_mi355x.decode(q, k, v, lens, causal=True) + 0

    with torch.no_grad():
        comp = torch.compile(f, backend="eager", fullgraph=True)(q, k, v, lens)
    assert torch.equal(comp, want)


def test_op_in_hip_graph_follows_lengths():
    """One linear capture, one replay; kv_lens changes between them."""
    import fa_mi355x.torch_op  # noqa: F401

    q, k, v = (dr.dev(a) for a in dr.inputs(1, 8, 2, 1, 2048, 128))
    lens = dr.lens([2048])
    for n in (2048, 700):  # eager references (and the first-launch set-up) outside the capture
        lens.fill_(n)
        torch.ops.fa_mi355x.decode(q, k, v, lens, True)
    want = torch.ops.fa_mi355x.decode(q, k, v, lens, True).clone()  # lens = 700
    lens.fill_(2048)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        torch.ops.fa_mi355x.decode(q, k, v, lens, True)  # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = torch.ops.fa_mi355x.decode(q, k, v, lens, True)
    lens.fill_(700)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, want)
