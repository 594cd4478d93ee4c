"""GPU tests of prefill attention over the K/V cache (fa_prefill_* /
fa_prefill_paged_* / fa_prefill_kv8_* / fa_prefill_paged_kv8_*: any Sq, GQA,
per-element kv_lens and q_lens, bottom-right causal, the four cache forms).

References and gates are the project's own (tests/decode_refs.py through
tests/prefill_refs.py), no new tolerance:
  * fp16 O: the CPU oracle per element with its n_b rows and len_b keys, 1e-3;
  * bf16 O: fp32 torch, 5e-3;
  * LSE: float64, 2^-10 * max|scaled score| + 1e-5;
  * kv8: against the dequantised cache (power-of-two per-head scales,
    exactness asserted, so the oracle applies);
  * rows that see no key: exactly 0 / -inf; rows t >= n_b: not written.
Shapes sit at the kernel's seams: the 128-row query block, the 32-row wave,
the 64-key tile and the page edge.
"""
import itertools

import numpy as np
import pytest
import torch

import decode_refs as dr
import fa_mi355x
import keysense_inputs as ks
import prefill_refs as pr

pytestmark = pytest.mark.gpu

DEV = "cuda"
FP8 = torch.float8_e4m3fn
PAD8 = 0x7f  # the E4M3 NaN
K_SCALE = (2.0 ** -6, 2.0 ** -3)
V_SCALE = (2.0 ** -4, 2.0 ** -8)
F16, BF16 = torch.float16, torch.bfloat16

prefill = fa_mi355x.flash_attention_prefill
prefill_paged = fa_mi355x.flash_attention_prefill_paged
decode = fa_mi355x.flash_attention_decode
decode_paged = fa_mi355x.flash_attention_decode_paged
append = fa_mi355x.flash_attention_cache_append
append_paged = fa_mi355x.flash_attention_cache_append_paged


def _scale_t(vals):
    return torch.tensor(list(vals), dtype=torch.float32, device=DEV)


def _pad(t, lens):
    """NaN bits in the cache rows at or past each length."""
    for i, n in enumerate(lens):
        t[i, :, int(n):].view(torch.int16).fill_(dr.NAN_BITS)
    return t


def _case(b, hq, hkv, sq, cap, d, kv_lens, dtype):
    """host (q, k, v) fp16 bits and device tensors of `dtype`, the caches' rows
    past each length NaN."""
    host = dr.inputs(b, hq, hkv, sq, cap, d)
    tq, tk, tv = (dr.dev(a).to(dtype) for a in host)
    clean = (tq, tk.clone(), tv.clone())  # the references never index past a length, but multiply
    return host, clean, (tq, _pad(tk, kv_lens), _pad(tv, kv_lens))


def _quant(x, scale):
    s = _scale_t(scale)[None, :, None, None]
    y = x / s
    assert float(y.abs().max()) <= 448.0
    x8 = y.to(FP8)
    assert bool(torch.isfinite(x8.float()).all())
    return x8, x8.float() * s


def _pad8(x8, lens):
    for i, n in enumerate(lens):
        x8[i, :, int(n):].view(torch.uint8).fill_(PAD8)
    return x8


def _case8(b, hq, hkv, sq, cap, d, kv_lens, dtype, k_scale=K_SCALE, v_scale=V_SCALE):
    """test_decode_kv8_gpu._case8 for any Sq: host / dev see the dequantised
    cache (exact in both 16-bit types, asserted), q8 is what the entry takes."""
    q, k, v = dr.inputs(b, hq, hkv, sq, cap, d)
    tq = dr.dev(q).to(dtype)
    k8, kd = _quant(dr.dev(k).float(), k_scale)
    v8, vd = _quant(dr.dev(v).float(), v_scale)
    for x in (kd, vd):
        assert torch.equal(x.to(F16).float(), x) and torch.equal(x.to(BF16).float(), x)
    host = (q, dr.bits(kd.to(F16)), dr.bits(vd.to(F16)))
    return host, (tq, kd.to(dtype), vd.to(dtype)), (tq, _pad8(k8, kv_lens), _pad8(v8, kv_lens))


def _paginate8(k8, v8, page_size, lens, **kw):
    kp, vp, table = dr.paginate(k8.view(torch.uint8), v8.view(torch.uint8), page_size, lens, **kw)
    return kp.view(FP8), vp.view(FP8), table


def _lens(vals):
    return None if vals is None else dr.lens(vals)


def _same_rows(a, b, q_lens):
    """Bit-equal (O, LSE) on the rows t < n_b of every element (the others are not written)."""
    return all(torch.equal(a[0][bi, :, :n], b[0][bi, :, :n]) and torch.equal(a[1][bi, :, :n], b[1][bi, :, :n])
               for bi, n in enumerate(q_lens))


def _raw(q, k, v, out, lse, kv_lens, q_lens, causal, table=None, scales=None):
    """The C entry itself, with the caller's own out AND lse buffers (the Python
    function allocates its LSE)."""
    lib = fa_mi355x.load_library()
    paged, kv8 = table is not None, k.dtype is FP8
    fn = getattr(lib, "fa_prefill" + ("_paged" if paged else "") + ("_kv8" if kv8 else "")
                 + ("_bf16" if q.dtype is BF16 else "_f16"))
    b, hq, sq, d = q.shape
    cache = (d, k.shape[0], k.shape[2], table.data_ptr(), table.shape[1]) if paged else (k.shape[2], d)
    tail = ()
    if kv8:
        tail = tuple(None if s is None else s.data_ptr() for s in (scales or (None, None)))
    rc = fn(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), lse.data_ptr(), b, hq, k.shape[1], sq,
            *cache, None if kv_lens is None else kv_lens.data_ptr(),
            None if q_lens is None else q_lens.data_ptr(), int(causal),
            torch.cuda.current_stream().cuda_stream, *tail)
    assert rc == fa_mi355x.FA_OK, rc
    torch.cuda.synchronize()


# ---- 1. the seam matrix, contiguous -------------------------------------------------

SQS = (1, 17, 127, 128, 129, 321)
HEADS = ((4, 4), (6, 2), (8, 1))
OFFS = (0, 63, 65, 300)
VARIANTS = list(itertools.product((F16, BF16), (128, 64), (True, False)))


def _seam_cases():
    """Every (Sq, heads) pair with three of the eight (dtype, D, causal)
    variants, rotating, plus all eight at (129, (6, 2)) and (321, (6, 2)):
    about 60 cases that touch every value of every axis; the prefixes rotate
    with the case."""
    seen, out = set(), []
    for idx, (sq, heads) in enumerate(itertools.product(SQS, HEADS)):
        picks = [(3 * idx + r) % 8 for r in range(3)]
        if heads == (6, 2) and sq in (129, 321):
            picks = range(8)
        for vi in picks:
            key = (sq, heads, vi)
            if key not in seen:
                seen.add(key)
                out.append(pytest.param(sq, heads, *VARIANTS[vi], idx + vi,
                                        id=f"Sq{sq}-H{heads[0]}x{heads[1]}-{dr.name(VARIANTS[vi][0])}-"
                                           f"d{VARIANTS[vi][1]}-{'causal' if VARIANTS[vi][2] else 'full'}"))
    return out


def _ragged(sq, rot):
    """q_lens (Sq, Sq - 1, 33 or 1) and kv_lens = prefix + n with three of the
    four prefixes."""
    q_lens = (sq, sq - 1, 33 if sq > 33 else 1)
    offs = [OFFS[(rot + i) % 4] for i in range(3)]
    return q_lens, tuple(o + n for o, n in zip(offs, q_lens))


@pytest.mark.parametrize("sq,heads,dtype,d,causal,rot", _seam_cases())
def test_seam_matrix(sq, heads, dtype, d, causal, rot):
    b, (hq, hkv), cap = 3, heads, 640
    q_lens, kv_lens = _ragged(sq, rot)
    host, clean, (tq, tk, tv) = _case(b, hq, hkv, sq, cap, d, kv_lens, dtype)
    refs = pr.refs(host, clean, kv_lens, q_lens, causal, dtype)
    out, lse = prefill(tq, tk, tv, _lens(kv_lens), _lens(q_lens), causal=causal, return_lse=True)
    pr.check(out, lse, refs, q_lens, dtype, f"seam Sq={sq} {heads} {dr.name(dtype)} d={d} causal={causal} "
                                            f"q_lens={q_lens} kv_lens={kv_lens}")


def test_lens_none_mean_full():
    """q_lens None = Sq rows, kv_lens None = the capacity (a 64-key multiple and not)."""
    for cap in (256, 200):
        host, clean, (tq, tk, tv) = _case(2, 4, 2, 130, cap, 128, (cap, cap), F16)
        refs = pr.refs(host, clean, None, None, True, F16)
        out, lse = prefill(tq, tk, tv, return_lse=True)
        pr.check(out, lse, refs, None, F16, f"lens None cap={cap}")
        assert dr.same(prefill(tq, tk, tv, _lens((cap, cap)), _lens((130, 130)), return_lse=True), (out, lse))


# ---- 2. rows and cache rows that are not touched ------------------------------------

@pytest.mark.parametrize("form", ["contig", "paged", "contig_kv8", "paged_kv8"])
@pytest.mark.parametrize("dtype", dr.DTYPES)
def test_untouched_rows(dtype, form):
    """out and lse pre-filled with NaN bits: rows t >= n_b keep their bits, every
    row below is finite.  Cache rows past len_b are NaN; paged: unused pages NaN
    and the table's filler arbitrary ids."""
    b, hq, hkv, sq, cap, d = 3, 6, 2, 200, 512, 128
    q_lens, kv_lens = (200, 129, 0), (263, 194, 70)
    kv8 = form.endswith("kv8")
    if kv8:
        host, clean, (tq, tk, tv) = _case8(b, hq, hkv, sq, cap, d, kv_lens, dtype)
        scales = (_scale_t(K_SCALE), _scale_t(V_SCALE))
    else:
        host, clean, (tq, tk, tv) = _case(b, hq, hkv, sq, cap, d, kv_lens, dtype)
        scales = None
    table = None
    if form.startswith("paged"):
        pg = _paginate8 if kv8 else dr.paginate
        tk, tv, table = pg(tk, tv, 128, kv_lens, seed=3, filler="junk")
    out = dr.nan_fill(torch.empty_like(tq))
    lse = torch.full((b, hq, sq), float("nan"), dtype=torch.float32, device=DEV)
    lse_bits = lse.view(torch.int32).clone()
    _raw(tq, tk, tv, out, lse, _lens(kv_lens), _lens(q_lens), True, table, scales)
    for bi, n in enumerate(q_lens):
        assert bool((out[bi, :, n:].view(torch.int16) == dr.NAN_BITS).all()), bi
        assert torch.equal(lse[bi, :, n:].view(torch.int32), lse_bits[bi, :, n:]), bi
        assert bool(torch.isfinite(out[bi, :, :n]).all()) and bool(torch.isfinite(lse[bi, :, :n]).all()), bi
    refs = pr.refs(host, clean, kv_lens, q_lens, True, dtype)
    pr.check(out, lse, refs, q_lens, dtype, f"untouched {form} {dr.name(dtype)}")


# ---- 3. paged == contiguous, bit for bit --------------------------------------------

@pytest.mark.parametrize("page_size", [64, 128, 256])
@pytest.mark.parametrize("d", [128, 64])
@pytest.mark.parametrize("dtype", dr.DTYPES)
def test_paged_bit_identical_to_contiguous(dtype, d, page_size):
    b, hq, hkv, sq, cap = 3, 6, 2, 200, 768
    q_lens, kv_lens = (200, 77, 130), (700, 140, 130)
    _, _, (tq, tk, tv) = _case(b, hq, hkv, sq, cap, d, kv_lens, dtype)
    kp, vp, table = dr.paginate(tk, tv, page_size, kv_lens, seed=page_size, filler="junk")
    gk, gv = dr.gather(kp, table), dr.gather(vp, table)
    for causal in (True, False):
        want = prefill(tq, gk, gv, _lens(kv_lens), _lens(q_lens), causal=causal, return_lse=True,
                       out=torch.zeros_like(tq))
        got = prefill_paged(tq, kp, vp, table, _lens(kv_lens), _lens(q_lens), causal=causal, return_lse=True,
                            out=torch.zeros_like(tq))
        for bi, n in enumerate(q_lens):
            assert torch.equal(got[0][bi, :, :n], want[0][bi, :, :n]), (bi, causal)
            assert torch.equal(got[1][bi, :, :n], want[1][bi, :, :n]), (bi, causal)
        assert bool(torch.isfinite(got[0]).all())


@pytest.mark.parametrize("kv8", [False, True], ids=["16bit", "kv8"])
def test_out_of_range_page_ids_read_as_zero_rows(kv8):
    """Ids -2, -1, num_pages, num_pages + 1 and INT_MAX in entries that ARE read
    give the bits of the contiguous entry on a cache with those rows zeroed.
    The pool is a slice of a larger NaN-filled allocation, two pages in from
    either end, so even a missing clamp reads only this test's memory."""
    b, hq, hkv, sq, cap, d = 2, 4, 2, 150, 384, 128
    q_lens, kv_lens = (150, 100), (320, 170)
    if kv8:
        _, _, (tq, tk, tv) = _case8(b, hq, hkv, sq, cap, d, kv_lens, F16)
        kp0, vp0, table = _paginate8(tk, tv, 64, kv_lens, seed=6)
        scales = dict(k_scale=_scale_t(K_SCALE), v_scale=_scale_t(V_SCALE))
    else:
        _, _, (tq, tk, tv) = _case(b, hq, hkv, sq, cap, d, kv_lens, F16)
        kp0, vp0, table = dr.paginate(tk, tv, 64, kv_lens, seed=6)
        scales = {}
    n = kp0.shape[0]
    shape = (n + 4,) + tuple(kp0.shape[1:])
    if kv8:
        bigk = torch.full(shape, 0xff, dtype=torch.uint8, device=DEV).view(FP8)
    else:
        bigk = dr.nan_fill(torch.empty(shape, dtype=F16, device=DEV))
    bigv = bigk.clone()
    kp, vp = bigk[2:2 + n], bigv[2:2 + n]
    kp.view(torch.uint8).copy_(kp0.view(torch.uint8))
    vp.view(torch.uint8).copy_(vp0.view(torch.uint8))
    assert kp.is_contiguous() and vp.is_contiguous()
    bad = table.clone()
    zk, zv = tk.clone(), tv.clone()
    for j, pid in zip(range(5), (-2, -1, n, n + 1, 2 ** 31 - 1)):  # element 0 reads entries 0..4
        bad[0, j] = pid
    for t in (zk, zv):
        t[0, :, :320].view(torch.uint8).zero_()
    want = prefill(tq, zk, zv, _lens(kv_lens), _lens(q_lens), return_lse=True, out=torch.zeros_like(tq), **scales)
    got = prefill_paged(tq, kp, vp, bad, _lens(kv_lens), _lens(q_lens), return_lse=True,
                        out=torch.zeros_like(tq), **scales)
    for bi, nq in enumerate(q_lens):
        assert torch.equal(got[0][bi, :, :nq], want[0][bi, :, :nq]), bi
        assert torch.equal(got[1][bi, :, :nq], want[1][bi, :, :nq]), bi
    assert bool(torch.isfinite(got[0]).all())
    # every key of element 0 is a zero row: O = 0, LSE = log(vis)
    assert int(torch.count_nonzero(got[0][0]).item()) == 0
    vis = torch.arange(171, 321, device=DEV, dtype=torch.float32)
    assert float((got[1][0] - torch.log(vis)[None, :]).abs().max()) <= 1e-5


# ---- 4. the FP8 cache ----------------------------------------------------------------

@pytest.mark.parametrize("d", [128, 64])
@pytest.mark.parametrize("dtype", dr.DTYPES)
def test_kv8_against_dequantised_references(dtype, d):
    """Per-head scales that differ between heads, contiguous and paged, causal and not."""
    b, hq, hkv, sq, cap = 3, 6, 2, 161, 512
    q_lens, kv_lens = (161, 160, 33), (161 + 65, 160, 33 + 300)
    host, dev, (tq, k8, v8) = _case8(b, hq, hkv, sq, cap, d, kv_lens, dtype)
    ksc, vsc = _scale_t(K_SCALE), _scale_t(V_SCALE)
    kp, vp, table = _paginate8(k8, v8, 128, kv_lens, seed=1, filler="junk")
    for causal in (True, False):
        refs = pr.refs(host, dev, kv_lens, q_lens, causal, dtype)
        tag = f"kv8 {dr.name(dtype)} d={d} causal={causal}"
        out, lse = prefill(tq, k8, v8, _lens(kv_lens), _lens(q_lens), causal=causal, return_lse=True,
                           k_scale=ksc, v_scale=vsc)
        pr.check(out, lse, refs, q_lens, dtype, "contig " + tag)
        out, lse = prefill_paged(tq, kp, vp, table, _lens(kv_lens), _lens(q_lens), causal=causal,
                                 return_lse=True, k_scale=ksc, v_scale=vsc)
        pr.check(out, lse, refs, q_lens, dtype, "paged " + tag)


@pytest.mark.parametrize("d", [128, 64])
@pytest.mark.parametrize("dtype", dr.DTYPES)
def test_kv8_none_scales_ones_and_16bit_cache(dtype, d):
    """Scales None = scales of ones, bit for bit; and with scales None the kv8
    entry equals the 16-bit entry on cache.to(dtype) bit for bit: every E4M3
    code is exact in both 16-bit types and the conversion happens before LDS,
    so the MFMA operands are identical."""
    b, hq, hkv, sq, cap = 2, 4, 2, 140, 320
    q_lens, kv_lens = (140, 139), (300, 139)
    one = (1.0, 1.0)
    _, _, (tq, k8, v8) = _case8(b, hq, hkv, sq, cap, d, kv_lens, dtype, one, one)
    ones = _scale_t(one)
    tl, ql = _lens(kv_lens), _lens(q_lens)
    want = prefill(tq, k8, v8, tl, ql, k_scale=ones, v_scale=ones, return_lse=True, out=torch.zeros_like(tq))
    for sc in ({}, {"v_scale": ones}, {"k_scale": ones}):
        assert _same_rows(prefill(tq, k8, v8, tl, ql, return_lse=True, **sc), want, q_lens), sc
    k16, v16 = k8.float().to(dtype), v8.float().to(dtype)  # NaN rows past the lengths stay NaN
    got = prefill(tq, k16, v16, tl, ql, return_lse=True, out=torch.zeros_like(tq))
    assert _same_rows(got, want, q_lens)
    kp, vp, table = _paginate8(k8, v8, 64, kv_lens, seed=9)
    pwant = prefill_paged(tq, kp, vp, table, tl, ql, return_lse=True, out=torch.zeros_like(tq),
                          k_scale=ones, v_scale=ones)
    assert _same_rows(prefill_paged(tq, kp, vp, table, tl, ql, return_lse=True), pwant, q_lens)
    assert _same_rows(pwant, want, q_lens)


# ---- 5. agreement with decode ---------------------------------------------------------

@pytest.mark.parametrize("sq", [1, 5, 16])
@pytest.mark.parametrize("dtype", dr.DTYPES)
def test_agrees_with_decode(dtype, sq):
    """q_lens None and Sq <= 16: the contract is decode's own.  Within the sum of
    the two gates (the reduction orders differ), on all four forms."""
    b, hq, hkv, cap, d = 3, 8, 2, 384, 128
    kv_lens = (70, 300, 384)
    tl = _lens(kv_lens)
    gate = 2 * (dr.GATE_F16 if dtype is F16 else dr.GATE_BF16)
    _, _, (tq, tk, tv) = _case(b, hq, hkv, sq, cap, d, kv_lens, dtype)
    _, _, (_, k8, v8) = _case8(b, hq, hkv, sq, cap, d, kv_lens, dtype)
    sc = dict(k_scale=_scale_t(K_SCALE), v_scale=_scale_t(V_SCALE))
    kp, vp, table = dr.paginate(tk, tv, 128, kv_lens, seed=2)
    kp8, vp8, table8 = _paginate8(k8, v8, 128, kv_lens, seed=2)
    smax = pr.lse_rows(tq, tk.nan_to_num(), tv, kv_lens, None, True)[1]
    pairs = {
        "contig": (prefill(tq, tk, tv, tl, return_lse=True), decode(tq, tk, tv, tl, return_lse=True)),
        "paged": (prefill_paged(tq, kp, vp, table, tl, return_lse=True),
                  decode_paged(tq, kp, vp, table, tl, return_lse=True)),
        "contig_kv8": (prefill(tq, k8, v8, tl, return_lse=True, **sc), decode(tq, k8, v8, tl, return_lse=True, **sc)),
        "paged_kv8": (prefill_paged(tq, kp8, vp8, table8, tl, return_lse=True, **sc),
                      decode_paged(tq, kp8, vp8, table8, tl, return_lse=True, **sc)),
    }
    for form, ((o1, l1), (o2, l2)) in pairs.items():
        err = float((o1.float() - o2.float()).abs().max())
        lerr = float((l1 - l2).abs().nan_to_num(posinf=float("inf")).max())
        print(f"{form} {dr.name(dtype)} Sq={sq}: |prefill - decode| O {err:.3e} LSE {lerr:.3e}")
        assert err <= gate, (form, err)
        assert torch.equal(torch.isneginf(l1), torch.isneginf(l2)), form
        fin = torch.isfinite(l2)
        assert float((l1[fin] - l2[fin]).abs().max()) <= 2 * (2.0 ** -10 * smax + 1e-5), form


# ---- 6. chunked prefill equals the whole ----------------------------------------------

@pytest.mark.parametrize("form", ["contig", "paged", "contig_kv8"])
@pytest.mark.parametrize("dtype", dr.DTYPES)
def test_chunked_equals_whole(dtype, form):
    """Prompts of 300 and 281 tokens (B = 2, Hq = 8, Hkv = 2) through append and
    prefill in chunks of 128, 128 and 44 / 25 against one append and one
    prefill: each chunk's O within the gate of the single-shot rows and of the
    reference, and on a 16-bit cache BIT-EQUAL to them: a chunk starts at a
    multiple of 128, so its rows sit in the same waves' lanes as in the
    single-shot block and meet the same keys in the same 64-key tiles in the
    same order.  (On the FP8 cache too: the appended bytes are the same.)"""
    b, hq, hkv, d, cap = 2, 8, 2, 128, 384
    total = (300, 281)
    q, k, v = dr.inputs(b, hq, hkv, 300, 300, d, seed=11)
    tq = dr.dev(q).to(dtype)
    knew = dr.dev(k).to(dtype)
    vnew = dr.dev(v).to(dtype)
    kv8, paged = form.endswith("kv8"), form.startswith("paged")
    sc = dict(k_scale=_scale_t((2.0 ** -6, 2.0 ** -5)), v_scale=_scale_t((2.0 ** -5, 2.0 ** -6))) if kv8 else {}

    def fresh():
        if paged:
            pool = dr.nan_fill(torch.empty((b * 3 + 2, hkv, 128, d), dtype=dtype, device=DEV))
            table = torch.tensor([[4, 1, 6], [0, 7, 3]], dtype=torch.int32, device=DEV)
            return pool, pool.clone(), table
        if kv8:
            c = torch.full((b, hkv, cap, d), PAD8, dtype=torch.uint8, device=DEV).view(FP8)
            return c, c.clone(), None
        c = dr.nan_fill(torch.empty((b, hkv, cap, d), dtype=dtype, device=DEV))
        return c, c.clone(), None

    def run(kc, vc, table, qx, kx, vx, kv_after, n_new):
        tl, nl = _lens(kv_after), _lens(n_new)
        if paged:
            append_paged(kx, vx, kc, vc, table, tl, nl, **sc)
            return prefill_paged(qx, kc, vc, table, tl, nl, return_lse=True, **sc)
        append(kx, vx, kc, vc, tl, nl, **sc)
        return prefill(qx, kc, vc, tl, nl, return_lse=True, **sc)

    kc, vc, table = fresh()
    whole = run(kc, vc, table, tq, knew, vnew, total, total)
    # the reference sees what the cache holds (the dequantised bytes for kv8)
    if kv8:
        ks_, vs_ = sc["k_scale"][None, :, None, None], sc["v_scale"][None, :, None, None]
        kd, vd = (kc.float() * ks_).nan_to_num().to(dtype), (vc.float() * vs_).nan_to_num().to(dtype)
        host = None
    else:
        kd, vd = (knew, vnew)
        host = (q, k, v) if dtype is F16 else None
        kd = torch.nn.functional.pad(kd, (0, 0, 0, cap - 300))
        vd = torch.nn.functional.pad(vd, (0, 0, 0, cap - 300))
        host = None if host is None else tuple(
            a if i == 0 else np.pad(a, ((0, 0), (0, 0), (0, cap - 300), (0, 0))) for i, a in enumerate(host))
    refs = pr.refs(host, (tq, kd, vd), total, total, True, dtype)
    pr.check(whole[0], whole[1], refs, total, dtype, f"whole {form} {dr.name(dtype)}")

    kc, vc, table = fresh()
    done = [0, 0]
    for size in (128, 128, 44):
        n_new = [min(size, t - s) for s, t in zip(done, total)]
        s0 = done[0]
        assert done[0] == done[1]
        sl = slice(s0, s0 + size)
        got = run(kc, vc, table, tq[:, :, sl].contiguous(), knew[:, :, sl].contiguous(),
                  vnew[:, :, sl].contiguous(), [s + n for s, n in zip(done, n_new)], n_new)
        for bi, n in enumerate(n_new):
            assert torch.equal(got[0][bi, :, :n], whole[0][bi, :, s0:s0 + n]), (size, bi)
            assert torch.equal(got[1][bi, :, :n], whole[1][bi, :, s0:s0 + n]), (size, bi)
        done = [s + size for s in done]


# ---- 7. unseen and short ---------------------------------------------------------------

@pytest.mark.parametrize("dtype", dr.DTYPES)
@pytest.mark.parametrize("causal", [True, False])
def test_unseen_and_short(dtype, causal):
    """kv_lens[b] < n_b (the leading rows see nothing), kv_lens[b] == 0,
    q_lens[b] == 0 (the element writes nothing), one key, one row."""
    b, hq, hkv, sq, cap, d = 5, 4, 2, 150, 256, 128
    q_lens = (150, 140, 0, 150, 1)
    kv_lens = (100, 0, 200, 1, 256)
    host, clean, (tq, tk, tv) = _case(b, hq, hkv, sq, cap, d, kv_lens, dtype)
    refs = pr.refs(host, clean, kv_lens, q_lens, causal, dtype)
    if causal:
        assert np.isneginf(refs[1][0, :, :50]).all() and np.isfinite(refs[1][0, :, 50:]).all()
        assert np.isneginf(refs[1][3, :, :149]).all() and np.isfinite(refs[1][3, :, 149:]).all()
    assert np.isneginf(refs[1][1, :, :140]).all()
    out = dr.nan_fill(torch.empty_like(tq))
    got, lse = prefill(tq, tk, tv, _lens(kv_lens), _lens(q_lens), causal=causal, out=out, return_lse=True)
    assert got is out
    pr.check(out, lse, refs, q_lens, dtype, f"unseen {dr.name(dtype)} causal={causal}")
    assert bool((out[2].view(torch.int16) == out[2].view(torch.int16)[0, 0, 0]).all())  # element 2: untouched
    assert bool(torch.isnan(out[2]).all()) and bool(torch.isnan(out[4, :, 1:]).all())


@pytest.mark.parametrize("paged", [False, True])
def test_zero_capacity(paged):
    """kv_capacity == 0: O = 0 and LSE = -inf for ALL rows, as decode does."""
    b, hq, hkv, sq, d = 2, 4, 2, 130, 64
    tq = dr.rand((b, hq, sq, d), F16, 1)
    out = dr.nan_fill(torch.empty_like(tq))
    if paged:
        pool = dr.rand((3, hkv, 64, d), F16, 2)
        table = torch.zeros((b, 0), dtype=torch.int32, device=DEV)
        got, lse = prefill_paged(tq, pool, pool, table, None, _lens((5, 130)), out=out, return_lse=True)
    else:
        cache = torch.empty((b, hkv, 0, d), dtype=F16, device=DEV)
        got, lse = prefill(tq, cache, cache, None, _lens((5, 130)), out=out, return_lse=True)
    assert int(torch.count_nonzero(got).item()) == 0 and bool(torch.isneginf(lse).all())


# ---- 8. key sensitivity ------------------------------------------------------------------

def _ks_forms(q, k, v, dtype):
    """The four forms' (O, LSE) on 16-bit inputs whose values are exact in E4M3."""
    tl, ql = _lens(pr.KS_KV_LENS), _lens(pr.KS_Q_LENS)
    k8, v8 = k.to(FP8), v.to(FP8)
    assert torch.equal(k8.to(dtype), k) and torch.equal(v8.to(dtype), v)
    kn, vn = _pad(k.clone(), pr.KS_KV_LENS), _pad(v.clone(), pr.KS_KV_LENS)
    k8, v8 = _pad8(k8, pr.KS_KV_LENS), _pad8(v8, pr.KS_KV_LENS)
    kp, vp, table = dr.paginate(kn, vn, 64, pr.KS_KV_LENS, seed=8, filler="junk")
    kp8, vp8, table8 = _paginate8(k8, v8, 192, pr.KS_KV_LENS, seed=8, filler="junk")
    yield "contig", prefill(q, kn, vn, tl, ql, return_lse=True)
    yield "paged", prefill_paged(q, kp, vp, table, tl, ql, return_lse=True)
    yield "contig_kv8", prefill(q, k8, v8, tl, ql, return_lse=True)
    yield "paged_kv8", prefill_paged(q, kp8, vp8, table8, tl, ql, return_lse=True)


@pytest.mark.parametrize("layout", ks.LAYOUTS)
@pytest.mark.parametrize("level", ks.LEVELS)
@pytest.mark.parametrize("d", [128, 64])
@pytest.mark.parametrize("dtype", dr.DTYPES)
def test_census(dtype, d, level, layout):
    """Q = K = level, V of zeros and ones: every row must count exactly its
    visible keys (vis of the contract) under the module's relative gate, at
    most half the 2^-6 signal of one wrong key (asserted in keysense_inputs)."""
    assert ks.REL_GATE[dtype] <= ks.SIGNAL / 2
    q, k, v, counts = pr.ks_census(level, layout, d, dtype, DEV)
    for form, (o, lse) in _ks_forms(q, k, v, dtype):
        pr.ks_check_census(o, lse, counts, level, layout, f"census {form} {dr.name(dtype)} d={d} {level} {layout}")


@pytest.mark.parametrize("kind", ["diagonal", "sweep"])
@pytest.mark.parametrize("d", [128, 64])
@pytest.mark.parametrize("dtype", dr.DTYPES)
def test_needle(dtype, d, kind):
    """diagonal: each row reads its last visible key off_b + t, so a bottom-right
    mask that is off by one spells the wrong index; sweep: earlier tiles."""
    q, k, v, pi, want = pr.ks_needle(kind, d, dtype, DEV)
    for form, (o, lse) in _ks_forms(q, k, v, dtype):
        pr.ks_check_needle(o, lse, q, k, pi, want, f"needle {kind} {form} {dr.name(dtype)} d={d}")


# ---- 9. plumbing -----------------------------------------------------------------------

def test_torch_ops_match_python_entries():
    import fa_mi355x.torch_op  # noqa: F401

    b, hq, hkv, sq, cap, d = 2, 8, 2, 140, 384, 128
    q_lens, kv_lens = (140, 140), (300, 140)
    _, _, (tq, tk, tv) = _case(b, hq, hkv, sq, cap, d, kv_lens, BF16)
    _, _, (_, k8, v8) = _case8(b, hq, hkv, sq, cap, d, kv_lens, BF16)
    tl, ql = _lens(kv_lens), _lens(q_lens)
    ksc, vsc = _scale_t(K_SCALE), _scale_t(V_SCALE)
    kp, vp, table = dr.paginate(tk, tv, 128, kv_lens, seed=2)
    kp8, vp8, table8 = _paginate8(k8, v8, 128, kv_lens, seed=2)
    op, opp = torch.ops.fa_mi355x.prefill, torch.ops.fa_mi355x.prefill_paged
    for causal in (True, False):
        want = prefill(tq, tk, tv, tl, ql, causal=causal)
        assert torch.equal(op(tq, tk, tv, tl, ql, causal), want)
        assert torch.equal(op(tq, tk, tv, kv_lens=tl, q_lens=ql, causal=causal), want)
        assert torch.equal(opp(tq, kp, vp, table, tl, ql, causal), want)
        want8 = prefill(tq, k8, v8, tl, ql, causal=causal, k_scale=ksc, v_scale=vsc)
        assert not torch.equal(want8, want)
        assert torch.equal(op(tq, k8, v8, tl, ql, causal, ksc, vsc), want8)
        assert torch.equal(opp(tq, kp8, vp8, table8, tl, ql, causal, k_scale=ksc, v_scale=vsc), want8)
    assert torch.equal(op(tq, tk, tv, tl), prefill(tq, tk, tv, tl))
    with pytest.raises(ValueError, match="needs GPU tensors"):
        op(tq.cpu(), tk.cpu(), tv.cpu())


def test_non_default_stream():
    b, hq, hkv, sq, cap, d = 2, 4, 2, 200, 320, 128
    q_lens, kv_lens = (200, 150), (300, 150)
    _, _, (tq, tk, tv) = _case(b, hq, hkv, sq, cap, d, kv_lens, F16)
    tl, ql = _lens(kv_lens), _lens(q_lens)
    want = prefill(tq, tk, tv, tl, ql, return_lse=True, out=torch.zeros_like(tq))
    s = torch.cuda.Stream()
    assert s.cuda_stream != torch.cuda.current_stream().cuda_stream
    s.wait_stream(torch.cuda.current_stream())
    out = torch.zeros_like(tq)
    got = prefill(tq, tk, tv, tl, ql, return_lse=True, out=out, stream=s)
    s.synchronize()
    assert got[0] is out and torch.equal(got[0], want[0])
    for bi, n in enumerate(q_lens):
        assert torch.equal(got[1][bi, :, :n], want[1][bi, :, :n])


def test_append_and_prefill_in_one_hip_graph_follow_device_values():
    """Append + prefill captured in one graph on one stream; before each replay
    kv_lens, q_lens and both scales are rewritten on the device: each replay
    gives the eager result of the values it finds."""
    b, hq, hkv, sq, cap, d = 2, 8, 2, 160, 512, 128
    q, k, v = dr.inputs(b, hq, hkv, sq, sq, d, seed=5)
    tq, kn, vn = (dr.dev(a) for a in (q, k, v))
    prefix = dr.inputs(b, hq, hkv, 1, cap, d, seed=6)
    kc0 = (dr.dev(prefix[1]).float() * 64).to(FP8)
    vc0 = (dr.dev(prefix[2]).float() * 64).to(FP8)
    kc, vc = kc0.clone(), vc0.clone()
    tl, ql = _lens((0, 0)), _lens((0, 0))
    ksc, vsc = _scale_t((1.0, 1.0)), _scale_t((1.0, 1.0))
    out = torch.zeros_like(tq)

    def step():
        append(kn, vn, kc, vc, tl, ql, k_scale=ksc, v_scale=vsc)
        return prefill(tq, kc, vc, tl, ql, out=out, k_scale=ksc, v_scale=vsc)

    def set_to(kvl, qls, a, bb):
        kc.copy_(kc0)
        vc.copy_(vc0)
        out.zero_()
        tl.copy_(_lens(kvl))
        ql.copy_(_lens(qls))
        ksc.copy_(_scale_t(a))
        vsc.copy_(_scale_t(bb))

    settings = [((400, 160), (160, 100), (2.0 ** -6, 2.0 ** -5), (2.0 ** -6, 2.0 ** -7)),
                ((230, 333), (31, 129), (2.0 ** -4, 2.0 ** -7), (2.0 ** -5, 2.0 ** -6))]
    wants = []
    for st in [((160, 160), (160, 160), (1.0, 1.0), (1.0, 1.0))] + settings:
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


@pytest.mark.skipif(not torch.cuda.is_available() or torch.cuda.device_count() < 2,
                    reason="needs two GPUs")
def test_non_current_device():
    """Tensors on cuda:1 while cuda:0 is current: the launch goes to cuda:1."""
    torch.cuda.set_device(0)
    d1 = torch.device("cuda", 1)
    _, _, (tq, tk, tv) = _case(1, 4, 2, 140, 192, 128, (192,), F16)
    want = prefill(tq, tk, tv)
    got = prefill(tq.to(d1), tk.to(d1), tv.to(d1))
    torch.cuda.synchronize(d1)
    assert got.device == d1 and torch.equal(got.cpu(), want.cpu())


def test_wrapper_rejections_on_device():
    _, _, (tq, tk, tv) = _case(2, 4, 2, 20, 64, 64, (64, 64), F16)
    with pytest.raises(fa_mi355x.FlashAttentionError, match="q_lens must be a tensor on"):
        prefill(tq, tk, tv, q_lens=torch.ones(2, dtype=torch.int32))
    with pytest.raises(fa_mi355x.FlashAttentionError, match="go with a torch.float8_e4m3fn cache only"):
        prefill(tq, tk, tv, k_scale=_scale_t((1.0, 1.0)))
