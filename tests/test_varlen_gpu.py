"""GPU tests of the packed (cu_seqlens, token-major) prefill and cache-append
entries (fa_prefill_varlen_* / fa_cache_append_varlen_*, all four cache forms).

The main gate is bit-identity with the padded entries on the unpacked tensors
(query blocks are aligned to each sequence's own start, so a workgroup runs
the padded entry's tile sequence); beside it the project's independent
references and gates through tests/prefill_refs.py on the unpacked result (fp16
O 1e-3 against the CPU oracle, bf16 O 5e-3 against fp32 torch, LSE 2^-10
max|score| + 1e-5), the key-sensitivity inputs, and sentinels around every
buffer.  No new tolerance.

The base shape is the smallest that crosses every seam of the map: B = 5,
n = (0, 1, 127, 128, 321) so cu = [0, 0, 1, 128, 256, 577] (an empty sequence,
a start off a 128 boundary, two starts on one), T = 600 > cu[B] (a tail of
rows that belong to no sequence), Hq = 8, Hkv = 2, prefixes (0, 200, 0, 70,
200) in caches of 576 rows.
"""
import functools

import numpy as np
import pytest
import torch

import decode_refs as dr
import fa_mi355x
import keysense_inputs as ks
import prefill_refs as pr
import varlen_refs as vr

pytestmark = pytest.mark.gpu

DEV = "cuda"
FP8 = torch.float8_e4m3fn
PAD8 = 0x7f  # the E4M3 NaN
K_SCALE = (2.0 ** -6, 2.0 ** -3)
V_SCALE = (2.0 ** -4, 2.0 ** -8)
F16, BF16 = torch.float16, torch.bfloat16
FORMS = ["contig", "paged", "contig_kv8", "paged_kv8"]

prefill = fa_mi355x.flash_attention_prefill
prefill_paged = fa_mi355x.flash_attention_prefill_paged
prefill_varlen = fa_mi355x.flash_attention_prefill_varlen
prefill_varlen_paged = fa_mi355x.flash_attention_prefill_varlen_paged
append = fa_mi355x.flash_attention_cache_append
append_paged = fa_mi355x.flash_attention_cache_append_paged
append_varlen = fa_mi355x.flash_attention_cache_append_varlen
append_varlen_paged = fa_mi355x.flash_attention_cache_append_varlen_paged

B, HQ, HKV, CAP, T = 5, 8, 2, 576, 600
N = (0, 1, 127, 128, 321)
PREFIX = (0, 200, 0, 70, 200)
KV_LENS = tuple(p + n for p, n in zip(PREFIX, N))
CU = vr.cu_of(N)
SMAX = max(N)
# the extra case: kv_lens[b] < n_b for elements 2 and 4 (off negative: leading rows see nothing)
KV_SHORT = (0, 201, 100, 198, 300)


def _scale_t(vals):
    return torch.tensor(list(vals), dtype=torch.float32, device=DEV)


def _lens(vals):
    return None if vals is None else dr.lens(vals)


def _pad(t, lens, cap_to=None):
    """NaN bits (PAD8 in an FP8 cache) in the rows at or past each length, the
    capacity grown to `cap_to` rows of the same."""
    one = t.element_size() == 1
    if cap_to is not None and cap_to > t.shape[2]:
        big = torch.empty(t.shape[:2] + (cap_to,) + t.shape[3:], dtype=t.dtype, device=t.device)
        big[:, :, :t.shape[2]] = t
        t = big
        lens = [min(int(n), t.shape[2]) for n in lens]
    else:
        t = t.clone()
    for i, n in enumerate(lens):
        rows = t[i, :, int(n):]
        if one:
            rows.view(torch.uint8).fill_(PAD8)
        else:
            rows.view(torch.int16).fill_(dr.NAN_BITS)
    return t


def _quant(x, scale):
    s = _scale_t(scale)[None, :, None, None]
    y = x / s
    assert float(y.abs().max()) <= 448.0
    x8 = y.to(FP8)
    assert bool(torch.isfinite(x8.float()).all())
    return x8, x8.float() * s


@functools.lru_cache(maxsize=None)
def _inputs(b, hq, hkv, smax, cap, d, dtype, kv8):
    """(host fp16 bits or None, clean device (q, k, v) the references read, the
    padded q, the caches the entries read (unpadded), scales or None).  kv8: the
    references see the dequantised cache (exact in both 16-bit types, asserted)."""
    q, k, v = dr.inputs(b, hq, hkv, smax, cap, d)
    tq = dr.dev(q).to(dtype)
    if not kv8:
        tk, tv = dr.dev(k).to(dtype), dr.dev(v).to(dtype)
        return (q, k, v), (tq, tk, tv), tq, (tk, tv), None
    k8, kd = _quant(dr.dev(k).float(), K_SCALE)
    v8, vd = _quant(dr.dev(v).float(), V_SCALE)
    for x in (kd, vd):
        assert torch.equal(x.to(F16).float(), x) and torch.equal(x.to(BF16).float(), x)
    host = (q, dr.bits(kd.to(F16)), dr.bits(vd.to(F16)))
    return host, (tq, kd.to(dtype), vd.to(dtype)), tq, (k8, v8), (_scale_t(K_SCALE), _scale_t(V_SCALE))


@functools.lru_cache(maxsize=None)
def _refs(b, hq, hkv, smax, cap, d, dtype, kv8, kv_lens, n, causal):
    """prefill_refs.refs on the padded tensors, computed once per case and shared."""
    host, clean, _, _, _ = _inputs(b, hq, hkv, smax, cap, d, dtype, kv8)
    return pr.refs(host, clean, kv_lens, n, causal, dtype)


def _paginate(k, v, page_size, lens, **kw):
    """dr.paginate of a cache whose capacity is first grown to a multiple of the page size."""
    cap = -(-k.shape[2] // page_size) * page_size
    k, v = _pad(k, lens, cap), _pad(v, lens, cap)
    if k.dtype is FP8:
        # (the pool's NaN-bit filler is the bytes 0xff 0x7f: both E4M3 NaN codes)
        kp, vp, table = dr.paginate(k.view(torch.uint8), v.view(torch.uint8), page_size, lens, **kw)
        return kp.view(FP8), vp.view(FP8), table
    return dr.paginate(k, v, page_size, lens, **kw)


def _both(form, tq, qp, caches, scales, kv_lens, n, cu, causal, page_size=64, seed=1, total=None):
    """(packed result unpacked to [B,Hq,Smax,D] / [B,Hq,Smax], padded result) of one
    cache form on the same cache, kv_lens and lengths."""
    tl, ql, tcu = _lens(kv_lens), _lens(n), _lens(cu)
    sc = {} if scales is None else dict(k_scale=scales[0], v_scale=scales[1])
    smax = tq.shape[2]
    if form.startswith("paged"):
        kp, vp, table = _paginate(*caches, page_size, kv_lens, seed=seed, filler="junk")
        got = prefill_varlen_paged(qp, kp, vp, table, tcu, tl, causal=causal, return_lse=True, **sc)
        want = prefill_paged(tq, kp, vp, table, tl, ql, causal=causal, return_lse=True, **sc)
    else:
        k, v = _pad(caches[0], kv_lens), _pad(caches[1], kv_lens)
        got = prefill_varlen(qp, k, v, tcu, tl, causal=causal, return_lse=True, **sc)
        want = prefill(tq, k, v, tl, ql, causal=causal, return_lse=True, **sc)
    assert got[0].shape == qp.shape and got[1].shape == (qp.shape[1], qp.shape[0])
    return (vr.unpack(got[0], cu, smax), vr.unpack(got[1], cu, smax, fill=float("-inf"))), want


def _same_rows(a, b, n):
    return all(torch.equal(a[0][bi, :, :nb], b[0][bi, :, :nb]) and torch.equal(a[1][bi, :, :nb], b[1][bi, :, :nb])
               for bi, nb in enumerate(n))


# ---- 1. bit-identical to the padded entry; 2. the independent references ---------------

@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("d", [128, 64])
@pytest.mark.parametrize("dtype", dr.DTYPES)
def test_bit_identical_to_padded_and_within_the_gates(dtype, d, form):
    """Rows t < n_b of O and LSE equal the padded entry's bit for bit, causal and
    not (paged: at page sizes 64, 128 and 256), and pass the project's gates
    against the references on their own."""
    kv8 = form.endswith("kv8")
    _, _, tq, caches, scales = _inputs(B, HQ, HKV, SMAX, CAP, d, dtype, kv8)
    qp = vr.pack(tq, N, total=T, fill=dr.NAN_BITS)
    for causal in (True, False):
        refs = _refs(B, HQ, HKV, SMAX, CAP, d, dtype, kv8, KV_LENS, N, causal)
        for ps in ((64, 128, 256) if form.startswith("paged") else (64,)):
            got, want = _both(form, tq, qp, caches, scales, KV_LENS, N, CU, causal, ps, seed=ps)
            what = f"{form} {dr.name(dtype)} d={d} causal={causal} page={ps}"
            assert _same_rows(got, want, N), what
            pr.check(got[0], got[1], refs, N, dtype, what)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("dtype", dr.DTYPES)
def test_lengths_shorter_than_the_chunk(dtype, form):
    """kv_lens[b] < n_b: off_b is negative and the leading rows see no key (0 / -inf)."""
    kv8 = form.endswith("kv8")
    _, _, tq, caches, scales = _inputs(B, HQ, HKV, SMAX, CAP, 128, dtype, kv8)
    qp = vr.pack(tq, N, total=T, fill=dr.NAN_BITS)
    refs = _refs(B, HQ, HKV, SMAX, CAP, 128, dtype, kv8, KV_SHORT, N, True)
    assert np.isneginf(refs[1][2, :, :27]).all() and np.isfinite(refs[1][2, :, 27:127]).all()
    assert np.isneginf(refs[1][4, :, :21]).all() and np.isfinite(refs[1][4, :, 21:]).all()
    got, want = _both(form, tq, qp, caches, scales, KV_SHORT, N, CU, True, 128)
    assert _same_rows(got, want, N)
    pr.check(got[0], got[1], refs, N, dtype, f"short {form} {dr.name(dtype)}")
    assert int(torch.count_nonzero(got[0][4, :, :21]).item()) == 0


# ---- 3. key sensitivity ----------------------------------------------------------------

KS_CU = vr.cu_of(pr.KS_Q_LENS)
assert KS_CU[-1] == 611


def _ks_forms(q, k, v, dtype):
    """The four packed forms' unpacked (O, LSE) on 16-bit inputs exact in E4M3."""
    tl, tcu = _lens(pr.KS_KV_LENS), _lens(KS_CU)
    qp = vr.pack(q, pr.KS_Q_LENS)
    k8, v8 = k.to(FP8), v.to(FP8)
    assert torch.equal(k8.to(dtype), k) and torch.equal(v8.to(dtype), v)
    kn, vn = _pad(k, pr.KS_KV_LENS), _pad(v, pr.KS_KV_LENS)
    k8, v8 = _pad(k8, pr.KS_KV_LENS), _pad(v8, pr.KS_KV_LENS)
    kp, vp, table = _paginate(kn, vn, 64, pr.KS_KV_LENS, seed=8, filler="junk")
    kp8, vp8, table8 = _paginate(k8, v8, 192, pr.KS_KV_LENS, seed=8, filler="junk")
    for form, res in (("contig", prefill_varlen(qp, kn, vn, tcu, tl, return_lse=True)),
                      ("paged", prefill_varlen_paged(qp, kp, vp, table, tcu, tl, return_lse=True)),
                      ("contig_kv8", prefill_varlen(qp, k8, v8, tcu, tl, return_lse=True)),
                      ("paged_kv8", prefill_varlen_paged(qp, kp8, vp8, table8, tcu, tl, return_lse=True))):
        yield form, (vr.unpack(res[0], KS_CU, pr.KS_SQ), vr.unpack(res[1], KS_CU, pr.KS_SQ, fill=float("-inf")))


@pytest.mark.parametrize("layout", ks.LAYOUTS)
@pytest.mark.parametrize("level", ks.LEVELS)
@pytest.mark.parametrize("d", [128, 64])
@pytest.mark.parametrize("dtype", dr.DTYPES)
def test_census(dtype, d, level, layout):
    """Every packed row counts exactly its visible keys (tests/test_prefill_gpu.py's
    census at B = 2, q_lens = (321, 290), packed into T = 611 rows)."""
    q, k, v, counts = pr.ks_census(level, layout, d, dtype, DEV)
    for form, (o, lse) in _ks_forms(q, k, v, dtype):
        pr.ks_check_census(o, lse, counts, level, layout,
                           f"varlen census {form} {dr.name(dtype)} d={d} {level} {layout}")


@pytest.mark.parametrize("kind", ["diagonal", "sweep"])
@pytest.mark.parametrize("d", [128, 64])
@pytest.mark.parametrize("dtype", dr.DTYPES)
def test_needle(dtype, d, kind):
    q, k, v, pi, want = pr.ks_needle(kind, d, dtype, DEV)
    for form, (o, lse) in _ks_forms(q, k, v, dtype):
        pr.ks_check_needle(o, lse, q, k, pi, want, f"varlen needle {kind} {form} {dr.name(dtype)} d={d}")


# ---- 4. rows that are not touched ------------------------------------------------------

def _raw(qp, k, v, out, lse, cu, kv_lens, causal, table=None, scales=None, nseq=None):
    """The C entry itself with the caller's own out AND lse buffers; returns the status."""
    lib = fa_mi355x.load_library()
    paged, kv8 = table is not None, k.dtype is FP8
    fn = getattr(lib, "fa_prefill_varlen" + ("_paged" if paged else "") + ("_kv8" if kv8 else "")
                 + ("_bf16" if qp.dtype is BF16 else "_f16"))
    total, hq, d = qp.shape
    cache = (d, k.shape[0], k.shape[2], table.data_ptr(), table.shape[1]) if paged else (k.shape[2], d)
    tail = ()
    if kv8:
        tail = tuple(None if s is None else s.data_ptr() for s in (scales or (None, None)))
    nseq = cu.shape[0] - 1 if nseq is None else nseq
    rc = fn(qp.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), None if lse is None else lse.data_ptr(),
            nseq, hq, k.shape[1], total, *cache, None if kv_lens is None else kv_lens.data_ptr(),
            cu.data_ptr(), int(causal), torch.cuda.current_stream().cuda_stream, *tail)
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("start", [0, 3])
@pytest.mark.parametrize("form", FORMS)
def test_untouched_rows(form, start):
    """O and LSE pre-filled with NaN bits: the rows [cu[B], T), the rows below
    cu[0] (start = 3) and nothing else keep them, for every head."""
    kv8 = form.endswith("kv8")
    _, _, tq, caches, scales = _inputs(B, HQ, HKV, SMAX, CAP, 128, F16, kv8)
    cu = vr.cu_of(N, start)
    qp = vr.pack(tq, N, total=T, start=start, fill=dr.NAN_BITS)
    out = dr.nan_fill(torch.empty_like(qp))
    lse = torch.full((HQ, T), float("nan"), dtype=torch.float32, device=DEV)
    lse_bits = lse.view(torch.int32).clone()
    if form.startswith("paged"):
        k, v, table = _paginate(*caches, 128, KV_LENS, seed=3, filler="junk")
    else:
        k, v, table = _pad(caches[0], KV_LENS), _pad(caches[1], KV_LENS), None
    assert _raw(qp, k, v, out, lse, _lens(cu), _lens(KV_LENS), True, table, scales) == fa_mi355x.FA_OK
    own = torch.from_numpy(vr.owned_rows(cu, T)).to(DEV)
    assert int(own.sum()) == 577 and not bool(own[577 + start:].any()) and not bool(own[:start].any())
    assert bool((out[~own].view(torch.int16) == dr.NAN_BITS).all())
    assert torch.equal(lse.view(torch.int32)[:, ~own], lse_bits[:, ~own])
    assert bool(torch.isfinite(out[own]).all()) and bool(torch.isfinite(lse[:, own]).all())
    refs = _refs(B, HQ, HKV, SMAX, CAP, 128, F16, kv8, KV_LENS, N, True)
    pr.check(vr.unpack(out, cu, SMAX), vr.unpack(lse, cu, SMAX, fill=float("-inf")), refs, N, F16,
             f"untouched {form} start={start}")


# ---- 5. the grid bound -----------------------------------------------------------------

@pytest.mark.parametrize("dtype,d", [(F16, 128), (BF16, 64)])
def test_many_short_sequences(dtype, d):
    """B = 40 with n_b in {0..3}: T / 128 + 40 = 40 ids, most sequences sharing one
    128-row stretch of the packed tensor."""
    b, cap = 40, 128
    rng = np.random.default_rng(40)
    n = tuple(int(x) for x in rng.integers(0, 4, b))
    assert {0, 1, 2, 3} <= set(n) and sum(n) < 128
    kv_lens = tuple(int(p) + nb for p, nb in zip(rng.integers(0, 100, b), n))
    cu, total = vr.cu_of(n), sum(n)
    _, _, tq, caches, _ = _inputs(b, HQ, HKV, 3, cap, d, dtype, False)
    qp = vr.pack(tq, n)
    got, want = _both("contig", tq, qp, caches, None, kv_lens, n, cu, True)
    assert _same_rows(got, want, n)
    pr.check(got[0], got[1], _refs(b, HQ, HKV, 3, cap, d, dtype, False, kv_lens, n, True), n, dtype,
             f"B=40 T={total} {dr.name(dtype)} d={d}")
    got, want = _both("paged", tq, qp, caches, None, kv_lens, n, cu, False, 64)
    assert _same_rows(got, want, n)


@pytest.mark.parametrize("dtype,d", [(F16, 64), (BF16, 128)])
def test_one_sequence_filling_its_blocks(dtype, d):
    """B = 1, T = n = 256: ids 0 and 1 are the two blocks, id 2 (= T / 128 + B - 1) returns."""
    n, kv_lens, cu = (256,), (300,), [0, 256]
    assert [vr.block_of(cu, 256, 128, i) for i in range(3)] == [(0, 0), (0, 1), None]
    _, _, tq, caches, _ = _inputs(1, HQ, HKV, 256, 320, d, dtype, False)
    qp = vr.pack(tq, n)
    for causal in (True, False):
        got, want = _both("contig", tq, qp, caches, None, kv_lens, n, cu, causal)
        assert _same_rows(got, want, n)
        pr.check(got[0], got[1], _refs(1, HQ, HKV, 256, 320, d, dtype, False, kv_lens, n, causal), n, dtype,
                 f"B=1 T=256 {dr.name(dtype)} d={d} causal={causal}")


# ---- 6. hostile cu_seqlens -------------------------------------------------------------

HOSTILE = [
    [-5, 40, 700, 650, 90, 2 ** 31 - 1],        # below 0, above T, decreasing, INT_MAX
    [600, 300, 0, -2 ** 31, 300, 100],          # decreasing from T down
    [2 ** 31 - 1] * 6,                          # everything past the end
    [-7, -7, -1, 0, 0, -2 ** 31],               # nothing at all
    [13, 77, 77, 401, 333, 599],                # in range, one step back
]


def _embed(t, margin, fill):
    """`t` as a view two `margin`s into a larger allocation filled with `fill` bytes."""
    big = torch.empty((t.shape[0] + 2 * margin,) + tuple(t.shape[1:]), dtype=t.dtype, device=DEV)
    big.view(torch.uint8).fill_(fill)
    inner = big[margin:margin + t.shape[0]]
    inner.view(torch.uint8).copy_(t.contiguous().view(torch.uint8))
    return big, inner


def _margins_keep(big, margin, fill):
    raw = big.view(torch.uint8)
    return bool((raw[:margin] == fill).all()) and bool((raw[-margin:] == fill).all())


@pytest.mark.parametrize("cu", HOSTILE, ids=lambda c: "cu" + str(HOSTILE.index(c)))
@pytest.mark.parametrize("form", ["contig", "paged_kv8"])
def test_hostile_cu_seqlens_prefill(form, cu):
    """Any cu is memory-safe: the clamps keep every address inside the T rows.  Q,
    O and LSE sit inside larger sentinel-filled allocations: the margins keep
    their bytes, the call returns FA_OK, and rows no clamped span covers keep
    the sentinel."""
    kv8 = form.endswith("kv8")
    _, _, tq, caches, scales = _inputs(B, HQ, HKV, SMAX, CAP, 128, F16, kv8)
    qbig, qp = _embed(vr.pack(tq, N, total=T), 64, 0x7e)
    obig, out = _embed(torch.empty_like(qp), 64, 0x5a)
    out.view(torch.uint8).fill_(0x5a)
    lbig = torch.full((HQ + 2, T), float("nan"), dtype=torch.float32, device=DEV)
    lbig.view(torch.int32).fill_(0x5a5a5a5a)
    lse = lbig[1:1 + HQ]
    assert qp.is_contiguous() and out.is_contiguous() and lse.is_contiguous()
    if form.startswith("paged"):
        k, v, table = _paginate(*caches, 64, KV_LENS, seed=4, filler="junk")
    else:
        k, v, table = _pad(caches[0], KV_LENS), _pad(caches[1], KV_LENS), None
    kc, vc = k.clone(), v.clone()
    assert _raw(qp, k, v, out, lse, _lens(cu), _lens(KV_LENS), True, table, scales) == fa_mi355x.FA_OK
    assert _margins_keep(qbig, 64, 0x7e) and _margins_keep(obig, 64, 0x5a)
    assert bool((lbig[0].view(torch.int32) == 0x5a5a5a5a).all())
    assert bool((lbig[-1].view(torch.int32) == 0x5a5a5a5a).all())
    own = torch.from_numpy(vr.owned_rows(cu, T)).to(DEV)
    assert bool((out[~own].view(torch.uint8) == 0x5a).all())
    assert bool((lse[:, ~own].view(torch.int32) == 0x5a5a5a5a).all())
    assert torch.equal(k.view(torch.uint8), kc.view(torch.uint8))
    assert torch.equal(v.view(torch.uint8), vc.view(torch.uint8))


# ---- 7. append -------------------------------------------------------------------------

def _fresh_cache(form, dtype, d, page_size=128):
    """Sentinel-filled caches (NaN bits / the E4M3 NaN) and, paged, a table with
    out-of-pool ids among the entries that are written through."""
    kv8 = form.endswith("kv8")
    if form.startswith("paged"):
        mpp = -(-CAP // page_size)
        npages = B * mpp + 3
        shape = (npages, HKV, page_size, d)
        table = torch.from_numpy(np.random.default_rng(page_size).permutation(npages)[:B * mpp]
                                 .reshape(B, mpp).astype(np.int32)).to(DEV)
    else:
        shape, table = (B, HKV, CAP, d), None
    if kv8:
        c = torch.full(shape, PAD8, dtype=torch.uint8, device=DEV).view(FP8)
    else:
        c = dr.nan_fill(torch.empty(shape, dtype=dtype, device=DEV))
    return c, c.clone(), table


def _expected_rows(kv_lens, n, cap):
    """bool [B, cap]: the cache rows of the contract, kv_lens[b] - n_b + t where that row exists."""
    m = np.zeros((len(n), cap), bool)
    for bi, (ln, nb) in enumerate(zip(kv_lens, n)):
        r = np.arange(ln - nb, ln)
        m[bi, r[(r >= 0) & (r < cap)]] = True
    return m


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("d", [128, 64])
@pytest.mark.parametrize("dtype", dr.DTYPES)
def test_append_equals_padded_append(dtype, d, form):
    """The packed append leaves the caches byte for byte as the padded append with
    new_lens = n does (the FP8 bytes included), on sentinel-filled caches: no
    other row is written.  Element 4's length runs past the capacity (its last
    rows do not exist) and, paged, element 3 writes through out-of-pool ids:
    both are dropped."""
    kv8, paged = form.endswith("kv8"), form.startswith("paged")
    q, k, v = dr.inputs(B, HQ, HKV, SMAX, SMAX, d, seed=17)
    kn, vn = dr.dev(k).to(dtype), dr.dev(v).to(dtype)
    kv_lens = KV_LENS[:4] + (CAP + 40,)
    sc = dict(k_scale=_scale_t(K_SCALE), v_scale=_scale_t(V_SCALE)) if kv8 else {}
    knp, vnp = vr.pack(kn, N, total=T, fill=dr.NAN_BITS), vr.pack(vn, N, total=T, fill=dr.NAN_BITS)
    tl, nl, tcu = _lens(kv_lens), _lens(N), _lens(CU)
    for ps in ((64, 128, 256) if paged else (0,)):
        kc, vc, table = _fresh_cache(form, dtype, d, ps)
        kw, vw = kc.clone(), vc.clone()
        before = kc.view(torch.uint8).clone()
        if paged:
            table[3, 0], table[3, 1] = -1, kc.shape[0]
            append_varlen_paged(knp, vnp, kc, vc, table, tcu, tl, **sc)
            append_paged(kn, vn, kw, vw, table, tl, nl, **sc)
        else:
            append_varlen(knp, vnp, kc, vc, tcu, tl, **sc)
            append(kn, vn, kw, vw, tl, nl, **sc)
        torch.cuda.synchronize()
        assert torch.equal(kc.view(torch.uint8), kw.view(torch.uint8)), (form, ps)
        assert torch.equal(vc.view(torch.uint8), vw.view(torch.uint8)), (form, ps)
        # the rows of the contract, and only they, changed
        changed = (kc.view(torch.uint8) != before).any(-1)
        if paged:
            cap_p = table.shape[1] * ps
            want = _expected_rows(kv_lens, N, cap_p)
            want[3, :min(2 * ps, cap_p)] = False  # through the two out-of-pool ids
            got = np.zeros_like(want)
            tab = table.cpu().numpy()
            ch = changed.cpu().numpy()  # [num_pages, Hkv, page_size]
            seen = np.zeros(kc.shape[0], bool)
            for bi in range(B):
                for j in range(tab.shape[1]):
                    if 0 <= tab[bi, j] < kc.shape[0]:
                        assert (ch[tab[bi, j]] == ch[tab[bi, j]][0]).all()  # every head alike
                        got[bi, j * ps:(j + 1) * ps] = ch[tab[bi, j], 0]
                        seen[tab[bi, j]] = True
            assert not ch[~seen].any(), (form, ps)
        else:
            want = _expected_rows(kv_lens, N, CAP)
            ch = changed.cpu().numpy()  # [B, Hkv, cap]
            assert (ch == ch[:, :1]).all()
            got = ch[:, 0]
        assert np.array_equal(got, want), (form, ps)
        if not kv8 and not paged:  # the bytes are the source's
            assert torch.equal(kc[4, :, 295:CAP], kn[4, :, :CAP - 295])  # row kv_lens - n + t = 295 + t
            assert torch.equal(vc[2, :, :127], vn[2, :, :127])


@pytest.mark.parametrize("cu", HOSTILE, ids=lambda c: "cu" + str(HOSTILE.index(c)))
@pytest.mark.parametrize("form", ["contig", "paged_kv8"])
def test_hostile_cu_seqlens_append(form, cu):
    """Any cu is memory-safe for the append too: k_new / v_new and the caches sit
    inside sentinel-filled allocations whose margins keep their bytes, and only
    the cache rows the clamped spans address change."""
    kv8 = form.endswith("kv8")
    q, k, v = dr.inputs(B, HQ, HKV, SMAX, SMAX, 128, seed=17)
    kn, vn = dr.dev(k), dr.dev(v)
    kbig, knp = _embed(vr.pack(kn, N, total=T), 64, 0x7e)
    vbig, vnp = _embed(vr.pack(vn, N, total=T), 64, 0x7e)
    kc0, vc0, table = _fresh_cache(form, F16, 128, 64)
    margin = 2
    fill = PAD8 if kv8 else 0x7f
    ckbig, kc = _embed(kc0, margin, fill)
    cvbig, vc = _embed(vc0, margin, fill)
    before = kc.view(torch.uint8).clone()
    sc = dict(k_scale=_scale_t(K_SCALE), v_scale=_scale_t(V_SCALE)) if kv8 else {}
    kv_lens = (576, 300, 250, 198, 521)
    if table is not None:
        append_varlen_paged(knp, vnp, kc, vc, table, _lens(cu), _lens(kv_lens), **sc)
    else:
        append_varlen(knp, vnp, kc, vc, _lens(cu), _lens(kv_lens), **sc)
    torch.cuda.synchronize()
    for big, m, f in ((kbig, 64, 0x7e), (vbig, 64, 0x7e), (ckbig, margin, fill), (cvbig, margin, fill)):
        assert _margins_keep(big, m, f)
    n = [nb for _, nb in vr.spans(cu, T)]
    want = _expected_rows(kv_lens, n, CAP)
    ch = (kc.view(torch.uint8) != before).any(-1).cpu().numpy()
    if table is None:
        got = ch[:, 0]
    else:
        tab = table.cpu().numpy()
        got = np.concatenate([ch[tab[:, j], 0] for j in range(tab.shape[1])], axis=1)
        seen = np.zeros(kc.shape[0], bool)
        seen[tab.flatten()] = True
        assert not ch[~seen].any()
    assert not (got & ~want).any(), cu  # nothing outside the addressed rows


# ---- 8. one captured graph ---------------------------------------------------------------

def test_append_and_prefill_in_one_hip_graph_follow_device_values():
    """append_varlen + prefill_varlen captured in one graph; before each replay cu
    and kv_lens are rewritten on the device (the same T, another split): each
    replay gives the eager result of the values it finds."""
    d, total, b = 128, 400, 3
    q, k, v = dr.inputs(1, HQ, HKV, total, total, d, seed=5)
    qp = dr.dev(q)[0].permute(1, 0, 2).contiguous()
    knp, vnp = (dr.dev(a)[0].permute(1, 0, 2).contiguous() for a in (k, v))
    prefix = dr.inputs(b, HQ, HKV, 1, CAP, d, seed=6)
    kc0, vc0 = dr.dev(prefix[1]), dr.dev(prefix[2])
    kc, vc = kc0.clone(), vc0.clone()
    tcu, tl = _lens([0] * (b + 1)), _lens([0] * b)
    out = torch.zeros_like(qp)

    def step():
        append_varlen(knp, vnp, kc, vc, tcu, tl)
        return prefill_varlen(qp, kc, vc, tcu, tl, out=out)

    def set_to(cu, kv_lens):
        kc.copy_(kc0)
        vc.copy_(vc0)
        out.zero_()
        tcu.copy_(_lens(cu))
        tl.copy_(_lens(kv_lens))

    settings = [([0, 130, 131, 400], (330, 1, 576)), ([5, 5, 261, 390], (77, 256, 400))]
    wants = []
    for st in [([0, 100, 200, 300], (100, 100, 100))] + settings:
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


# ---- 9. plumbing -------------------------------------------------------------------------

def test_torch_ops_match_python_entries():
    import fa_mi355x.torch_op  # noqa: F401

    ops = torch.ops.fa_mi355x
    _, _, tq, (tk, tv), _ = _inputs(B, HQ, HKV, SMAX, CAP, 128, BF16, False)
    _, _, _, (k8, v8), (ksc, vsc) = _inputs(B, HQ, HKV, SMAX, CAP, 128, BF16, True)
    qp = vr.pack(tq, N, total=T)
    tl, tcu = _lens(KV_LENS), _lens(CU)
    kp, vp, table = _paginate(tk, tv, 128, KV_LENS, seed=2)
    kp8, vp8, table8 = _paginate(k8, v8, 128, KV_LENS, seed=2)
    own = torch.from_numpy(vr.owned_rows(CU, T)).to(DEV)
    for causal in (True, False):
        want = prefill_varlen(qp, tk, tv, tcu, tl, causal=causal)[own]
        assert torch.equal(ops.prefill_varlen(qp, tk, tv, tcu, tl, causal)[own], want)
        assert torch.equal(ops.prefill_varlen(qp, tk, tv, cu_seqlens_q=tcu, kv_lens=tl, causal=causal)[own], want)
        assert torch.equal(ops.prefill_varlen_paged(qp, kp, vp, table, tcu, tl, causal)[own], want)
        want8 = prefill_varlen(qp, k8, v8, tcu, tl, causal=causal, k_scale=ksc, v_scale=vsc)[own]
        assert not torch.equal(want8, want)
        assert torch.equal(ops.prefill_varlen(qp, k8, v8, tcu, tl, causal, ksc, vsc)[own], want8)
        assert torch.equal(ops.prefill_varlen_paged(qp, kp8, vp8, table8, tcu, tl, causal, k_scale=ksc,
                                                    v_scale=vsc)[own], want8)
    with pytest.raises(ValueError, match="needs GPU tensors"):
        ops.prefill_varlen(qp.cpu(), tk.cpu(), tv.cpu(), tcu.cpu())
    # the append ops
    knp = vr.pack(tk[:, :, :SMAX].contiguous(), N, total=T)
    for form in FORMS:
        kv8 = form.endswith("kv8")
        sc = (ksc, vsc) if kv8 else (None, None)
        kc, vc, tab = _fresh_cache(form, BF16, 128)
        kw, vw = kc.clone(), vc.clone()
        if tab is not None:
            ops.cache_append_varlen_paged(knp, knp, kc, vc, tab, tcu, tl, *sc)
            append_varlen_paged(knp, knp, kw, vw, tab, tcu, tl, k_scale=sc[0], v_scale=sc[1])
        else:
            ops.cache_append_varlen(knp, knp, kc, vc, tcu, tl, *sc)
            append_varlen(knp, knp, kw, vw, tcu, tl, k_scale=sc[0], v_scale=sc[1])
        assert torch.equal(kc.view(torch.uint8), kw.view(torch.uint8)), form
        assert torch.equal(vc.view(torch.uint8), vw.view(torch.uint8)), form
        assert not torch.equal(kc.view(torch.uint8), _fresh_cache(form, BF16, 128)[0].view(torch.uint8))


def test_non_default_stream():
    _, _, tq, (tk, tv), _ = _inputs(B, HQ, HKV, SMAX, CAP, 128, F16, False)
    qp = vr.pack(tq, N, total=T)
    tl, tcu = _lens(KV_LENS), _lens(CU)
    want = prefill_varlen(qp, tk, tv, tcu, tl, return_lse=True, out=torch.zeros_like(qp))
    kw, vw, _ = _fresh_cache("contig", F16, 128)
    append_varlen(qp[:, :HKV].contiguous(), qp[:, HKV:2 * HKV].contiguous(), kw, vw, tcu, tl)
    s = torch.cuda.Stream()
    assert s.cuda_stream != torch.cuda.current_stream().cuda_stream
    s.wait_stream(torch.cuda.current_stream())
    out = torch.zeros_like(qp)
    got = prefill_varlen(qp, tk, tv, tcu, tl, return_lse=True, out=out, stream=s)
    kc, vc, _ = _fresh_cache("contig", F16, 128)
    s.wait_stream(torch.cuda.current_stream())
    append_varlen(qp[:, :HKV].contiguous(), qp[:, HKV:2 * HKV].contiguous(), kc, vc, tcu, tl, stream=s)
    s.synchronize()
    own = torch.from_numpy(vr.owned_rows(CU, T)).to(DEV)
    assert got[0] is out and torch.equal(got[0], want[0])
    assert torch.equal(got[1][:, own], want[1][:, own])
    assert torch.equal(kc.view(torch.int16), kw.view(torch.int16))
    assert torch.equal(vc.view(torch.int16), vw.view(torch.int16))


def test_wrapper_rejections_on_device():
    _, _, tq, (tk, tv), _ = _inputs(B, HQ, HKV, SMAX, CAP, 128, F16, False)
    qp = vr.pack(tq, N, total=T)
    err = fa_mi355x.FlashAttentionError
    with pytest.raises(err, match="cu_seqlens_q must be a tensor on cuda"):
        prefill_varlen(qp, tk, tv, torch.tensor(CU, dtype=torch.int32))
    with pytest.raises(err, match=r"cu_seqlens_q must be a contiguous \[B \+ 1 = 6\] tensor, got \[5\]"):
        prefill_varlen(qp, tk, tv, _lens(CU[:5]))
    with pytest.raises(err, match="kv_lens must be a tensor on cuda"):
        prefill_varlen(qp, tk, tv, _lens(CU), torch.tensor(KV_LENS, dtype=torch.int32))
    with pytest.raises(err, match="go with a torch.float8_e4m3fn cache only"):
        prefill_varlen(qp, tk, tv, _lens(CU), k_scale=_scale_t((1.0, 1.0)))
    kn = qp[:, :HKV].contiguous()
    with pytest.raises(err, match="cu_seqlens must be a tensor on cuda"):
        append_varlen(kn, kn, tk.clone(), tv.clone(), torch.tensor(CU, dtype=torch.int32), _lens(KV_LENS))
    with pytest.raises(err, match="kv_lens is required"):
        append_varlen(kn, kn, tk.clone(), tv.clone(), _lens(CU), None)


@pytest.mark.parametrize("paged", [False, True])
def test_zero_capacity(paged):
    """kv_capacity == 0: O = 0 and LSE = -inf for ALL T rows, as the padded entry does."""
    d = 64
    qp = dr.rand((T, HQ, d), F16, 1)
    out = dr.nan_fill(torch.empty_like(qp))
    if paged:
        pool = dr.rand((3, HKV, 64, d), F16, 2)
        table = torch.zeros((B, 0), dtype=torch.int32, device=DEV)
        got, lse = prefill_varlen_paged(qp, pool, pool, table, _lens(CU), out=out, return_lse=True)
        append_varlen_paged(qp[:, :HKV].contiguous(), qp[:, :HKV].contiguous(), pool, pool.clone(), table,
                            _lens(CU), _lens(KV_LENS))
    else:
        cache = torch.empty((B, HKV, 0, d), dtype=F16, device=DEV)
        got, lse = prefill_varlen(qp, cache, cache, _lens(CU), out=out, return_lse=True)
        append_varlen(qp[:, :HKV].contiguous(), qp[:, :HKV].contiguous(), cache, cache, _lens(CU),
                      _lens(KV_LENS))
    assert got is out and lse.shape == (HQ, T)
    assert int(torch.count_nonzero(got).item()) == 0 and bool(torch.isneginf(lse).all())


def test_no_tokens():
    """T == 0: FA_OK, nothing launched, empty results of the right shapes."""
    _, _, _, (tk, tv), _ = _inputs(B, HQ, HKV, SMAX, CAP, 128, F16, False)
    qp = torch.empty((0, HQ, 128), dtype=F16, device=DEV)
    cu = _lens([0] * (B + 1))
    out, lse = prefill_varlen(qp, tk, tv, cu, _lens(KV_LENS), return_lse=True)
    assert out.shape == (0, HQ, 128) and lse.shape == (HQ, 0)
    kc = tk.clone()
    kn = torch.empty((0, HKV, 128), dtype=F16, device=DEV)
    append_varlen(kn, kn, kc, tv.clone(), cu, _lens(KV_LENS))
    torch.cuda.synchronize()
    assert torch.equal(kc, tk)
