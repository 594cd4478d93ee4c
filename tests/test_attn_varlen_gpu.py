"""GPU tests of the fa_attn_varlen_* entries: attention over token-major Q
[T_q, Hq, D] and K, V [T_k, Hkv, D] with no cache (ragged by cu_seqlens_q /
cu_seqlens_k, self-attention, uniform [B, S, H, D]), GQA, runtime strides,
sliding window and sinks.

The main gate is bit-identity of O and LSE with flash_attention_prefill_varlen
on a contiguous cache whose rows [0, nk_b) are sequence b's keys (kv_lens =
nk): the same block alignment and tile sequence, hence the same bits.  Beside
it the project's references and gates through tests/prefill_refs.py,
window_refs.py and sink_refs.py on the unpacked result (fp16 O 1e-3 against
the CPU oracle, bf16 O 5e-3 against fp32 torch, LSE 2^-10 max|score| + 1e-5),
the key-sensitivity inputs, and sentinels around every buffer.  No new
tolerance.  The base shape is tests/attn_varlen_refs.py's.
"""
import functools

import numpy as np
import pytest
import torch

import attn_varlen_refs as ar
import decode_refs as dr
import fa_mi355x
import keysense_inputs as ks
import prefill_refs as pr
import sink_refs as sr
import varlen_refs as vr
import window_refs as wr

pytestmark = pytest.mark.gpu

DEV = "cuda"
F16, BF16 = torch.float16, torch.bfloat16
B, HQ, HKV, NQ, NK, TQ, TK = ar.B, ar.HQ, ar.HKV, ar.NQ, ar.NK, ar.TQ, ar.TK
CU_Q, CU_K, SMAX, CAP = ar.CU_Q, ar.CU_K, ar.SMAX, ar.CAP

attn = fa_mi355x.flash_attention_varlen
bshd = fa_mi355x.flash_attention_bshd
prefill_varlen = fa_mi355x.flash_attention_prefill_varlen
lens = dr.lens


@functools.lru_cache(maxsize=None)
def _base(d, dtype):
    """(packed q, k, v with NaN bits in the rows of no sequence; the NaN-padded
    caches the reference call reads)."""
    _, dev = ar.padded(d, dtype)
    return ar.packed(dev), (ar.nan_cache(dev[1], NK), ar.nan_cache(dev[2], NK))


def _twin(qp, caches, cu_q, nk, causal, **kw):
    """The reference call, unpacked."""
    o, lse = prefill_varlen(qp, caches[0], caches[1], lens(cu_q), lens(nk), causal=causal, return_lse=True, **kw)
    return ar.unpack(o, lse, cu_q)


# ---- 1. the base sweep -------------------------------------------------------------------

@pytest.mark.parametrize("d", [128, 64])
@pytest.mark.parametrize("dtype", dr.DTYPES)
def test_base_sweep(dtype, d):
    """Bit-identical to the cache twin and within the gates, causal and not, with
    NaN bits in every K/V row of no sequence; O and LSE rows of no sequence keep
    their sentinel bits."""
    (qp, kp, vp), caches = _base(d, dtype)
    own = torch.from_numpy(vr.owned_rows(CU_Q, TQ)).to(DEV)
    kown = torch.from_numpy(vr.owned_rows(CU_K, TK)).to(DEV)
    assert bool((kp[~kown].view(torch.int16) == dr.NAN_BITS).all()) and int((~kown).sum()) == TK - 1027
    for causal in (True, False):
        what = f"attn_varlen {dr.name(dtype)} d={d} causal={causal}"
        out = dr.nan_fill(torch.empty_like(qp))
        lse = torch.empty((HQ, TQ), dtype=torch.float32, device=DEV)
        lse.view(torch.int32).fill_(0x7fc01234)
        assert ar.raw("", qp, kp, vp, out, lse, lens(CU_Q), lens(CU_K), causal) == fa_mi355x.FA_OK
        assert bool((out[~own].view(torch.int16) == dr.NAN_BITS).all()), what
        assert bool((lse[:, ~own].view(torch.int32) == 0x7fc01234).all()), what
        assert bool(torch.isfinite(out[own]).all()), what
        got = ar.unpack(out, lse)
        assert ar.same_rows(got, _twin(qp, caches, CU_Q, NK, causal), NQ), what
        pr.check(got[0], got[1], ar.refs(d, dtype, causal), NQ, dtype, what)
        # the wrapper: the same bits
        o2, l2 = attn(qp, kp, vp, lens(CU_Q), lens(CU_K), causal=causal, return_lse=True)
        assert o2.shape == qp.shape and l2.shape == (HQ, TQ)
        assert torch.equal(o2[own], out[own]) and torch.equal(l2[:, own], lse[:, own]), what
    # off_b < 0 for element 2 (100 keys, 127 rows): its first 27 rows see nothing when causal
    r = ar.refs(d, dtype, True)
    assert np.isneginf(r[1][2, :, :27]).all() and np.isfinite(r[1][2, :, 27:127]).all()


# ---- 2. self-attention ---------------------------------------------------------------------

@pytest.mark.parametrize("dtype", dr.DTYPES)
def test_self_attention(dtype):
    """cu_seqlens_k=None with nk = nq (K, V packed like Q): the explicit form's bits."""
    d = 128
    host, dev = ar.padded(d, dtype)
    qp = vr.pack(dev[0], NQ, total=TQ, fill=dr.NAN_BITS)
    kp, vp = (vr.pack(x[:, :, :SMAX].contiguous(), NQ, total=TQ, fill=dr.NAN_BITS) for x in dev[1:])
    caches = (ar.nan_cache(dev[1], NQ), ar.nan_cache(dev[2], NQ))
    own = torch.from_numpy(vr.owned_rows(CU_Q, TQ)).to(DEV)
    for causal in (True, False):
        a = attn(qp, kp, vp, lens(CU_Q), None, causal=causal, return_lse=True)
        e = attn(qp, kp, vp, lens(CU_Q), lens(CU_Q), causal=causal, return_lse=True)
        assert torch.equal(a[0][own], e[0][own]) and torch.equal(a[1][:, own], e[1][:, own])
        got = ar.unpack(*a)
        assert ar.same_rows(got, _twin(qp, caches, CU_Q, NQ, causal), NQ)
        pr.check(got[0], got[1], pr.refs(host, dev, NQ, NQ, causal, dtype), NQ, dtype,
                 f"self {dr.name(dtype)} causal={causal}")


@pytest.mark.parametrize("causal", [True, False])
def test_a_sequence_without_keys(causal):
    """nk_b = 0 < nq_b (element 3): zeros and -inf for its 128 rows, the others as ever."""
    d, dtype = 64, F16
    nk = (7, 201, 100, 0, 521)
    cu_k = vr.cu_of(nk, 3)
    host, dev = ar.padded(d, dtype)
    qp, kp, vp = ar.packed(dev, nk=nk)
    o, lse = attn(qp, kp, vp, lens(CU_Q), lens(cu_k), causal=causal, return_lse=True)
    assert int(torch.count_nonzero(o[128:256]).item()) == 0 and bool(torch.isneginf(lse[:, 128:256]).all())
    assert bool(torch.isfinite(lse[:, 256:577]).all())
    got = ar.unpack(o, lse)
    caches = (ar.nan_cache(dev[1], nk), ar.nan_cache(dev[2], nk))
    assert ar.same_rows(got, _twin(qp, caches, CU_Q, nk, causal), NQ)
    pr.check(got[0], got[1], pr.refs(host, dev, nk, NQ, causal, dtype), NQ, dtype, f"no keys causal={causal}")


# ---- 3. strided input ----------------------------------------------------------------------

@pytest.mark.parametrize("d", [128, 64])
@pytest.mark.parametrize("dtype", dr.DTYPES)
def test_fused_qkv_buffer_read_in_place(dtype, d):
    """Q, K and V as the three head slices of one [T, Hq + 2 Hkv, D] buffer of NaN
    bits: the dense call's bits, into a dense out."""
    (qp, kp, vp), _ = _base(d, dtype)
    fq, fk, fv = ar.fused_qkv(qp, kp, vp)
    assert fq.stride(0) == fk.stride(0) == fv.stride(0) == (HQ + 2 * HKV) * d and not fk.is_contiguous()
    own = torch.from_numpy(vr.owned_rows(CU_Q, TQ)).to(DEV)
    for causal in (True, False):
        want = attn(qp, kp, vp, lens(CU_Q), lens(CU_K), causal=causal, return_lse=True)
        got = attn(fq, fk, fv, lens(CU_Q), lens(CU_K), causal=causal, return_lse=True)
        assert got[0].is_contiguous() and got[0].shape == qp.shape
        assert torch.equal(got[0][own], want[0][own]) and torch.equal(got[1][:, own], want[1][:, own])


def test_strides_that_are_refused():
    (qp, kp, vp), _ = _base(64, F16)
    err = fa_mi355x.FlashAttentionError
    odd = torch.zeros(TK * 132 + 8, dtype=F16, device=DEV).as_strided((TK, HKV, 64), (132, 64, 1))
    with pytest.raises(err, match="k: the token stride 132 must be a multiple of 8 elements"):
        attn(qp, odd, vp, lens(CU_Q), lens(CU_K))
    wide = torch.zeros((TK, HKV, 128), dtype=F16, device=DEV)[:, :, ::2]
    with pytest.raises(err, match=r"v must have stride\(-1\) == 1 and stride\(-2\) == head_dim"):
        attn(qp, kp, wide, lens(CU_Q), lens(CU_K))
    # the entry itself refuses them too, before any launch
    out = torch.empty_like(qp)
    fn = ar.entry(fa_mi355x.load_library(), "", False)
    args = (qp.data_ptr(), kp.data_ptr(), vp.data_ptr(), out.data_ptr(), None, B, HQ, HKV, TQ, TK, 64,
            lens(CU_Q).data_ptr(), lens(CU_K).data_ptr(), True)
    assert ar.call(fn, "", *args, strides=(0, 132, 0)) == fa_mi355x.FA_ERR_BAD_SHAPE
    assert ar.call(fn, "", *args, strides=(0, 0, 64)) == fa_mi355x.FA_ERR_BAD_SHAPE


# ---- 4. uniform mode -----------------------------------------------------------------------

@pytest.mark.parametrize("dtype,d", [(F16, 128), (BF16, 64)])
def test_bshd_equals_varlen_with_explicit_cu(dtype, d):
    """flash_attention_bshd (no cu array) at B = 3, Sq = 130, Sk = 200 and at Sq = Sk
    = 1: flash_attention_varlen with cu = arange * S, bit for bit; within the gates."""
    for b, sq, sk in ((3, 130, 200), (3, 1, 1)):
        host, dev = ar.padded(d, dtype, b=b, smax=sq, cap=sk, seed=11)
        q4, k4, v4 = (x.permute(0, 2, 1, 3).contiguous() for x in dev)   # [B,S,H,D]
        cu_q, cu_k = [i * sq for i in range(b + 1)], [i * sk for i in range(b + 1)]
        for causal in (True, False):
            o, lse = bshd(q4, k4, v4, causal=causal, return_lse=True)
            assert o.shape == (b, sq, HQ, d) and o.is_contiguous() and lse.shape == (b, HQ, sq)
            wo, wl = attn(q4.view(b * sq, HQ, d), k4.view(b * sk, HKV, d), v4.view(b * sk, HKV, d),
                          lens(cu_q), lens(cu_k), causal=causal, return_lse=True)
            assert torch.equal(o.view(b * sq, HQ, d), wo)
            assert torch.equal(lse, wl.view(HQ, b, sq).permute(1, 0, 2))
            pr.check(o.permute(0, 2, 1, 3), lse, pr.refs(host, dev, None, None, causal, dtype), None, dtype,
                     f"bshd {dr.name(dtype)} d={d} Sq={sq} Sk={sk} causal={causal}")


def test_bshd_reads_a_sliced_projection_output():
    """q, k, v as slices of one [B, S, (Hq + 2 Hkv) D] tensor: the contiguous call's bits."""
    b, s, d = 2, 150, 128
    _, dev = ar.padded(d, BF16, b=b, smax=s, cap=s, seed=12)
    q4, k4, v4 = (x.permute(0, 2, 1, 3).contiguous() for x in dev)
    proj = dr.nan_fill(torch.empty((b, s, (HQ + 2 * HKV) * d), dtype=BF16, device=DEV))
    views = (proj[..., :HQ * d].unflatten(-1, (HQ, d)), proj[..., HQ * d:(HQ + HKV) * d].unflatten(-1, (HKV, d)),
             proj[..., (HQ + HKV) * d:].unflatten(-1, (HKV, d)))
    for dst, src in zip(views, (q4, k4, v4)):
        dst.copy_(src)
    assert torch.equal(bshd(*views, causal=True), bshd(q4, k4, v4, causal=True))


# ---- 5. window and sinks ---------------------------------------------------------------------

@pytest.mark.parametrize("window", [1, 64, 200])
@pytest.mark.parametrize("dtype", dr.DTYPES)
def test_window_and_sinks(dtype, window):
    """The _win and _sink entries against window_refs / sink_refs and their cache
    twins bit for bit."""
    d = 128
    (qp, kp, vp), caches = _base(d, dtype)
    host, dev = ar.padded(d, dtype)
    what = f"{dr.name(dtype)} W={window}"
    got = ar.unpack(*attn(qp, kp, vp, lens(CU_Q), lens(CU_K), causal=True, return_lse=True, window=window))
    assert ar.same_rows(got, _twin(qp, caches, CU_Q, NK, True, window=window), NQ), what
    pr.check(got[0], got[1], wr.refs(host, dev, NK, NQ, window, dtype), NQ, dtype, "win " + what)
    sinks = sr.draw_sinks(HQ).to(DEV)
    sinks[3] = float("-inf")
    got = ar.unpack(*attn(qp, kp, vp, lens(CU_Q), lens(CU_K), causal=True, return_lse=True, window=window,
                          sinks=sinks))
    assert ar.same_rows(got, _twin(qp, caches, CU_Q, NK, True, window=window, sinks=sinks), NQ), what
    sr.check(got[0], got[1], sr.refs(host, dev, NK, NQ, window, dtype, sinks), NQ, dtype, "sink " + what)
    # element 2's leading rows see no key: zeros, and LSE = the head's sink (sink_refs' gate, above)
    assert int(torch.count_nonzero(got[0][2, :, :27]).item()) == 0
    assert bool(torch.isneginf(got[1][2, 3, :27]).all()) and bool(torch.isfinite(got[1][2, :3, :27]).all())


@pytest.mark.parametrize("dtype", dr.DTYPES)
def test_variant_equalities(dtype):
    """_sink with NULL sinks = _win; _win with W = 0 = the plain entry; sinks without a
    window and without causal against sink_refs."""
    d = 64
    (qp, kp, vp), caches = _base(d, dtype)
    host, dev = ar.padded(d, dtype)
    cq, ck = lens(CU_Q), lens(CU_K)
    own = torch.from_numpy(vr.owned_rows(CU_Q, TQ)).to(DEV)

    def run(variant, causal, window=0, sinks=None):
        out = torch.zeros_like(qp)
        lse = torch.zeros((HQ, TQ), dtype=torch.float32, device=DEV)
        assert ar.raw(variant, qp, kp, vp, out, lse, cq, ck, causal, window, sinks) == fa_mi355x.FA_OK
        return out, lse

    def same(a, b):
        return torch.equal(a[0][own], b[0][own]) and torch.equal(a[1][:, own].view(torch.int32),
                                                                 b[1][:, own].view(torch.int32))

    for causal in (True, False):
        assert same(run("_win", causal, 0), run("", causal)), causal
        assert same(run("_sink", causal, 0, None), run("", causal)), causal
    assert same(run("_sink", True, 64, None), run("_win", True, 64))
    assert not same(run("_win", True, 64), run("", True))
    none = torch.full((HQ,), float("-inf"), device=DEV)
    assert same(run("_sink", True, 64, none), run("_win", True, 64))
    sinks = sr.draw_sinks(HQ, seed=6).to(DEV)
    got = ar.unpack(*attn(qp, kp, vp, cq, ck, causal=False, return_lse=True, sinks=sinks))
    assert ar.same_rows(got, _twin(qp, caches, CU_Q, NK, False, sinks=sinks), NQ)
    sr.check(got[0], got[1], sr.refs(host, dev, NK, NQ, 0, dtype, sinks, causal=False), NQ, dtype,
             f"sinks non-causal {dr.name(dtype)}")


# ---- 6. key sensitivity ----------------------------------------------------------------------

def _vis(causal=True):
    """int64 [B, 1, Smax] vis of the contract at the base shape (rows t >= n_b: 0)."""
    return torch.from_numpy(np.maximum(pr.visible(NK, NQ, B, SMAX, CAP, causal), 0))[:, None, :]


@pytest.mark.parametrize("layout", ks.LAYOUTS)
@pytest.mark.parametrize("level", ks.LEVELS)
@pytest.mark.parametrize("dtype,d", [(F16, 128), (BF16, 64)])
def test_census(dtype, d, level, layout):
    """Every row counts exactly its visible keys: one lost, doubled or mis-masked key fails."""
    q, k, v, counts = ks.census_qkv((B, HQ, SMAX, d), (B, HKV, CAP, d), level, layout, dtype, DEV)
    qp, kp, vp = ar.packed((q, k, v))
    for causal in (True, False):
        o, lse = ar.unpack(*attn(qp, kp, vp, lens(CU_Q), lens(CU_K), causal=causal, return_lse=True))
        vis = _vis(causal)
        for bi, n in enumerate(NQ):
            if n:
                ks.check_census(o[bi, :, :n], vis[bi, :, :n], counts, level, layout,
                                f"attn census {dr.name(dtype)} d={d} {level} {layout} causal={causal} b={bi}",
                                lse=lse[bi, :, :n], dtype=dtype).require()


def _needle_targets(kind):
    """pi int64 [B, Hq, Smax]: "diagonal" the row's last visible key, "sweep" an
    earlier one (prefill_refs.ks_needle_targets' rule); -1 where the row sees none."""
    vis = _vis(True).numpy()[:, 0, :]
    t = np.arange(SMAX)[None, None, :]
    h = np.arange(HQ)[None, :, None]
    v3 = np.broadcast_to(vis[:, None, :], (B, HQ, SMAX))
    if kind == "diagonal":
        pi = v3 - 1
    else:
        tiles = np.maximum(-(-v3 // ks.TILE), 1)
        pi = np.minimum(((7 * t + 3 * h) % tiles) * ks.TILE + (5 * t + h) % ks.TILE, v3 - 1)
    return np.where(v3 > 0, pi, -1).astype(np.int64)


@pytest.mark.parametrize("kind", ["diagonal", "sweep"])
@pytest.mark.parametrize("dtype,d", [(F16, 64), (BF16, 128)])
def test_needle(dtype, d, kind):
    """Each row's query singles out one key: O must be that key's value."""
    k, v = ks.needle_kv((B, HKV), CAP, d, 7, dtype, DEV)
    pi = torch.from_numpy(_needle_targets(kind))
    g = HQ // HKV
    q, want = ks.needle_q(k, pi, g), ks.needle_expected(v, pi, g)
    qp, kp, vp = ar.packed((q, k, v))
    o, lse = ar.unpack(*attn(qp, kp, vp, lens(CU_Q), lens(CU_K), causal=True, return_lse=True))
    lref = ks.needle_lse_ref(q, k, _vis(True).expand(B, HQ, SMAX))
    for bi, n in enumerate(NQ):
        if n:
            ks.check_needle(o[bi, :, :n], want[bi, :, :n], pi[bi, :, :n],
                            f"attn needle {kind} {dr.name(dtype)} d={d} b={bi}", lse=lse[bi, :, :n],
                            lse_ref=lref[bi, :, :n], d=d).require()


# ---- 7. garbage cu_seqlens -------------------------------------------------------------------

HOSTILE = [
    [-5, 40, 700, 650, 90, 2 ** 31 - 1],        # below 0, above T, decreasing, INT_MAX
    [600, 300, 0, -2 ** 31, 300, 100],          # decreasing from T down
    [2 ** 31 - 1] * 6,                          # everything past the end
    [-7, -7, -1, 0, 0, -2 ** 31],               # nothing at all
    [13, 77, 77, 401, 333, 1099],               # in range, one step back
]


def _embed(t, margin, fill):
    """`t` as a view `margin` rows into a larger allocation filled with `fill` bytes."""
    big = torch.empty((t.shape[0] + 2 * margin,) + tuple(t.shape[1:]), dtype=t.dtype, device=DEV)
    big.view(torch.uint8).fill_(fill)
    inner = big[margin:margin + t.shape[0]]
    inner.copy_(t)
    return big, inner


def _margins_keep(big, margin, fill):
    raw = big.view(torch.uint8)
    return bool((raw[:margin] == fill).all()) and bool((raw[-margin:] == fill).all())


@pytest.mark.parametrize("which", ["q", "k", "both"])
@pytest.mark.parametrize("cu", HOSTILE, ids=lambda c: "cu" + str(HOSTILE.index(c)))
def test_hostile_cu_seqlens(cu, which):
    """Any cu_seqlens_q / cu_seqlens_k is memory-safe: the clamps keep every address
    inside the tensors' rows.  Q, K, V, O and LSE sit inside larger sentinel-filled
    allocations: the margins keep their bytes, the call returns FA_OK, O and LSE
    rows no clamped query span covers keep the sentinel, and K and V are unchanged."""
    (qp, kp, vp), _ = _base(128, F16)
    cu_q = cu if which in ("q", "both") else CU_Q
    cu_k = cu if which in ("k", "both") else CU_K
    qbig, q = _embed(qp, 64, 0x7e)
    kbig, k = _embed(kp, 64, 0x7e)
    vbig, v = _embed(vp, 64, 0x7e)
    obig, out = _embed(torch.empty_like(qp), 64, 0x5a)
    out.view(torch.uint8).fill_(0x5a)
    lbig = torch.empty((HQ + 2, TQ), dtype=torch.float32, device=DEV)
    lbig.view(torch.int32).fill_(0x5a5a5a5a)
    lse = lbig[1:1 + HQ]
    kc, vc = k.clone(), v.clone()
    assert ar.raw("", q, k, v, out, lse, lens(cu_q), lens(cu_k), True) == fa_mi355x.FA_OK
    for big, fill in ((qbig, 0x7e), (kbig, 0x7e), (vbig, 0x7e), (obig, 0x5a)):
        assert _margins_keep(big, 64, fill)
    assert bool((lbig[0].view(torch.int32) == 0x5a5a5a5a).all())
    assert bool((lbig[-1].view(torch.int32) == 0x5a5a5a5a).all())
    own = torch.from_numpy(vr.owned_rows(cu_q, TQ)).to(DEV)
    assert bool((out[~own].view(torch.uint8) == 0x5a).all())
    assert bool((lse[:, ~own].view(torch.int32) == 0x5a5a5a5a).all())
    assert torch.equal(k.view(torch.int16), kc.view(torch.int16))
    assert torch.equal(v.view(torch.int16), vc.view(torch.int16))


# ---- 8. past 4 GiB ---------------------------------------------------------------------------

def test_keys_past_4_gib():
    """K and V [2_100_300, 8, 128] fp16 (4.3 GB each): cu_seqlens_k = [2_100_000,
    2_100_300] puts the sequence's first key 2_100_000 * 2048 bytes > 2^32 into
    them; 300 queries, against the references."""
    hkv, d, start, n = 8, 128, 2_100_000, 300
    assert start * hkv * d * 2 > 2 ** 32
    host, dev = ar.padded(d, F16, b=1, hq=HQ, hkv=hkv, smax=n, cap=n, seed=21)
    qp = vr.pack(dev[0], (n,))
    kp = torch.empty((start + n, hkv, d), dtype=F16, device=DEV)
    vp = torch.empty((start + n, hkv, d), dtype=F16, device=DEV)
    # NaN bits in the rows next to the sequence (the bulk stays as allocated: never read)
    for x, src in ((kp, dev[1]), (vp, dev[2])):
        x[start - 4096:start].view(torch.int16).fill_(dr.NAN_BITS)
        x[start:] = src[0].permute(1, 0, 2)
    for causal in (True, False):
        o, lse = attn(qp, kp, vp, lens([0, n]), lens([start, start + n]), causal=causal, return_lse=True)
        got = ar.unpack(o, lse, [0, n], n)
        pr.check(got[0], got[1], pr.refs(host, dev, (n,), (n,), causal, F16), (n,), F16, f"4 GiB causal={causal}")
        assert ar.same_rows(got, _twin(qp, dev[1:], [0, n], (n,), causal), (n,))
    del kp, vp
    torch.cuda.empty_cache()


# ---- 9. torch ops, one graph, plumbing ---------------------------------------------------------

def test_torch_ops_match_python_functions():
    import fa_mi355x.torch_op  # noqa: F401

    ops = torch.ops.fa_mi355x
    (qp, kp, vp), _ = _base(128, BF16)
    fq, fk, fv = ar.fused_qkv(qp, kp, vp)
    cq, ck = lens(CU_Q), lens(CU_K)
    own = torch.from_numpy(vr.owned_rows(CU_Q, TQ)).to(DEV)
    sinks = sr.draw_sinks(HQ).to(DEV)
    for causal in (True, False):
        want = attn(qp, kp, vp, cq, ck, causal=causal)[own]
        assert torch.equal(ops.attn_varlen(qp, kp, vp, cq, ck, causal)[own], want)
        assert torch.equal(ops.attn_varlen(fq, fk, fv, cu_seqlens_q=cq, cu_seqlens_k=ck, causal=causal)[own], want)
        want = attn(qp, kp, vp, cq, ck, causal=causal, sinks=sinks)[own]
        assert torch.equal(ops.attn_varlen(qp, kp, vp, cq, ck, causal, 0, sinks)[own], want)
    want = attn(qp, kp, vp, cq, ck, causal=True, window=64)[own]
    assert torch.equal(ops.attn_varlen(qp, kp, vp, cq, ck, True, 64)[own], want)
    assert torch.equal(ops.attn_varlen(qp, kp, vp, cq, ck, True, window=64)[own], want)
    want = attn(qp, kp, vp, cq, ck, causal=True, window=64, sinks=sinks)[own]
    assert torch.equal(ops.attn_varlen(qp, kp, vp, cq, ck, True, window=64, sinks=sinks)[own], want)
    # self-attention (cu_seqlens_k omitted) on strided views: K and V are head slices of q
    ksf, vsf = qp[:, :HKV], qp[:, HKV:2 * HKV]
    assert torch.equal(ops.attn_varlen(qp, ksf, vsf, cq)[own], attn(qp, ksf, vsf, cq)[own])
    _, dev = ar.padded(128, BF16, b=2, smax=70, cap=90, seed=13)
    q4, k4, v4 = (x.permute(0, 2, 1, 3).contiguous() for x in dev)
    assert torch.equal(ops.attn_bshd(q4, k4, v4), bshd(q4, k4, v4))
    assert torch.equal(ops.attn_bshd(q4, k4, v4, True), bshd(q4, k4, v4, causal=True))
    assert torch.equal(ops.attn_bshd(q4, k4, v4, True, 16), bshd(q4, k4, v4, causal=True, window=16))
    assert torch.equal(ops.attn_bshd(q4, k4, v4, True, 16, sinks), bshd(q4, k4, v4, causal=True, window=16,
                                                                         sinks=sinks))
    with pytest.raises(ValueError, match="needs GPU tensors"):
        ops.attn_varlen(qp.cpu(), kp.cpu(), vp.cpu(), cq.cpu())


def test_one_hip_graph_follows_cu_rewritten_on_the_device():
    """flash_attention_varlen captured once; cu_seqlens_q and cu_seqlens_k are rewritten
    on the device before each replay: each replay gives the eager result of the values it finds."""
    qp, kp, vp = dr.rand((TQ, HQ, 128), F16, 31), dr.rand((TK, HKV, 128), F16, 32), dr.rand((TK, HKV, 128), F16, 33)
    cq, ck = lens([0] * (B + 1)), lens([0] * (B + 1))
    out = torch.zeros_like(qp)

    def step():
        return attn(qp, kp, vp, cq, ck, causal=True, out=out)

    def set_to(cu_q, cu_k):
        out.zero_()
        cq.copy_(lens(cu_q))
        ck.copy_(lens(cu_k))

    settings = [(CU_Q, CU_K), ([0, 130, 131, 400, 400, 600], [0, 300, 301, 800, 900, 1100])]
    wants = []
    for st in [([0, 100, 200, 300, 400, 500], [0, 100, 200, 300, 400, 500])] + settings:
        set_to(*st)
        wants.append(step().clone())
    assert not torch.equal(wants[1], wants[2]) and not torch.equal(wants[0], wants[1])
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()  # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    for st, want in zip(settings, wants[1:]):
        set_to(*st)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, want), st


def test_no_keys_at_all_and_no_tokens():
    """total_k == 0: O = 0 and LSE = -inf (with sinks: the sink) for ALL T_q rows;
    total_q == 0: FA_OK, empty results."""
    d = 64
    qp = dr.rand((TQ, HQ, d), F16, 1)
    kv = torch.empty((0, HKV, d), dtype=F16, device=DEV)
    o, lse = attn(qp, kv, kv, lens(CU_Q), lens([0] * (B + 1)), out=dr.nan_fill(torch.empty_like(qp)), return_lse=True)
    assert int(torch.count_nonzero(o).item()) == 0 and bool(torch.isneginf(lse).all())
    sinks = sr.draw_sinks(HQ).to(DEV)
    o, lse = attn(qp, kv, kv, lens(CU_Q), None, return_lse=True, sinks=sinks)
    assert int(torch.count_nonzero(o).item()) == 0 and torch.equal(lse, sinks[:, None].expand(HQ, TQ))
    (_, kp, vp), _ = _base(d, F16)
    o, lse = attn(qp[:0], kp, vp, lens([0] * (B + 1)), lens(CU_K), return_lse=True)
    assert o.shape == (0, HQ, d) and lse.shape == (HQ, 0)
    o = bshd(qp[:0].view(0, 5, HQ, d), kv.view(0, 7, HKV, d), kv.view(0, 7, HKV, d))
    assert o.shape == (0, 5, HQ, d)
