"""GPU tests of prefill, packed prefill and cache append in the two regimes
their own test files never reach: scores peaked enough that the lazy rescale
of the softmax runs (and stops short of running) with mass still on the
earlier tiles, and tensors whose byte offsets pass 4 GiB.

No new tolerance: fp16 O 1e-3, bf16 O 5e-3, LSE 2^-10 max|score| + 1e-5,
unseen rows exactly 0 / -inf, rows past n_b not written (decode_refs /
prefill_refs).  fp16 O on a 16-bit cache (and on an FP8 cache with
power-of-two scales, whose dequantised values are exact in fp16) is judged by
the CPU oracle; bf16 O and every FP8 case with a non-power-of-two scale by
prefill_refs.contract_f64 on float64(code) * float64(scale).  The staircase
inputs come from prefill_refs.staircase; tests/test_prefill_cpu.py holds, on
the CPU, which side of the rescale threshold their steps lie on, that every
value is exact in every type, and that the references alone use at most half
of each gate.

The tests past 4 GiB allocate with torch.empty and write only the rows they
use; lengths of zero keep the kernels off everything else.  None holds more
than about 10 GiB, and each frees its tensors at its end.
"""
import functools

import numpy as np
import pytest
import torch

import decode_refs as dr
import fa_mi355x
import fp8_contract
import prefill_refs as pr
import varlen_refs as vr

pytestmark = pytest.mark.gpu

DEV = "cuda"
FP8 = torch.float8_e4m3fn
PAD8 = 0x7f  # the E4M3 NaN
F16, BF16 = torch.float16, torch.bfloat16
K_SCALE = (2.0 ** -6, 2.0 ** -3)
V_SCALE = (2.0 ** -4, 2.0 ** -8)
WRAP = 1 << 32
# eight per-head FP8 scales, none a power of two (the tests past 4 GiB)
A_SCALES = ((0.013, 0.021, 0.034, 0.055, 0.089, 0.144, 0.233, 0.377),
            (0.377, 0.233, 0.144, 0.089, 0.055, 0.034, 0.021, 0.013))

prefill = fa_mi355x.flash_attention_prefill
prefill_paged = fa_mi355x.flash_attention_prefill_paged
prefill_varlen = fa_mi355x.flash_attention_prefill_varlen
prefill_varlen_paged = fa_mi355x.flash_attention_prefill_varlen_paged
decode = fa_mi355x.flash_attention_decode
decode_paged = fa_mi355x.flash_attention_decode_paged
append = fa_mi355x.flash_attention_cache_append
append_paged = fa_mi355x.flash_attention_cache_append_paged
append_varlen = fa_mi355x.flash_attention_cache_append_varlen
append_varlen_paged = fa_mi355x.flash_attention_cache_append_varlen_paged


def _scale_t(vals):
    return torch.tensor([float(x) for x in vals], dtype=torch.float32, device=DEV)


def _lens(vals):
    return None if vals is None else dr.lens(vals)


def _pad(t, lens):
    """A copy with NaN bits (the E4M3 NaN in an FP8 cache) in the rows at or past each length."""
    t = t.clone()
    for i, n in enumerate(lens):
        if t.element_size() == 1:
            t[i, :, int(n):].view(torch.uint8).fill_(PAD8)
        else:
            t[i, :, int(n):].view(torch.int16).fill_(dr.NAN_BITS)
    return t


def _paginate(k, v, page_size, lens, **kw):
    if k.dtype is FP8:
        kp, vp, table = dr.paginate(k.view(torch.uint8), v.view(torch.uint8), page_size, lens, **kw)
        return kp.view(FP8), vp.view(FP8), table
    return dr.paginate(k, v, page_size, lens, **kw)


def _nan_bits(t):
    """Whether every element of the 16-bit tensor t still holds the NaN pre-fill."""
    return bool((t.view(torch.int16) == dr.NAN_BITS).all())


def _same_rows(a, b, q_lens):
    """Bit-equal (O, LSE) on the rows t < n_b of every element (the others are not written)."""
    return all(torch.equal(a[0][bi, :, :n], b[0][bi, :, :n]) and torch.equal(a[1][bi, :, :n], b[1][bi, :, :n])
               for bi, n in enumerate(q_lens))


def _refs(tq, kd, vd, kv_lens, q_lens, causal, oracle):
    """The references of one case as prefill_refs.check takes them.  kd, vd: what
    the cache holds, dequantised (16-bit tensors, or float64 ones).  LSE and the
    largest score from contract_f64; O from the CPU oracle (fp16 inputs only)
    or from contract_f64."""
    o64, lse64, _, smax = pr.contract_f64(*(t.double().cpu().numpy() for t in (tq, kd, vd)), kv_lens, q_lens,
                                          causal, with_smax=True)
    if oracle:
        assert tq.dtype is F16 and kd.dtype is F16 and vd.dtype is F16
        return pr.oracle_rows(dr.bits(tq), dr.bits(kd), dr.bits(vd), kv_lens, q_lens, causal), lse64, smax
    return torch.tensor(np.nan_to_num(o64)).to(DEV), lse64, smax


# ---- 1. staircase inputs: the lazy rescale from both sides of its threshold --------------

@functools.lru_cache(maxsize=None)
def _st(pattern, d, carry, dtype):
    """Device tensors of prefill_refs.staircase at the ST_* shape: q, the 16-bit
    caches (carry "q" only), the FP8 caches and their scales (ones with carry
    "q"); cache rows past each length are NaN."""
    st = pr.staircase(pattern, d, carry)
    tq = torch.tensor(st.q).to(dtype).to(DEV)
    k8, v8 = (torch.tensor(a).float().to(FP8).to(DEV) for a in (st.k, st.v))
    for t8, a in ((k8, st.k), (v8, st.v)):
        assert torch.equal(t8.float().double().cpu(), torch.tensor(a))
    k16 = v16 = None
    if carry == "q":
        k16, v16 = (_pad(torch.tensor(a).to(dtype).to(DEV), pr.ST_KV_LENS) for a in (st.k, st.v))
    return tq, k16, v16, _pad(k8, pr.ST_KV_LENS), _pad(v8, pr.ST_KV_LENS), _scale_t(st.k_scale), _scale_t(st.v_scale)


@functools.lru_cache(maxsize=None)
def _st_refs(pattern, d, carry, causal, oracle):
    """(O, LSE, max score) of the staircase, shared by both dtypes (their inputs
    hold the same values): prefill_refs.st_contract, O from the CPU oracle
    where `oracle` (fp16 with the values the cache holds exact in fp16)."""
    o64, lse64, smax = pr.st_contract(pattern, d, carry, causal)
    if oracle:
        assert carry == "q"
        st = pr.staircase(pattern, d, carry)
        host = tuple(dr.bits(torch.tensor(a).to(F16)) for a in (st.q, st.k, st.v))
        return pr.oracle_rows(*host, pr.ST_KV_LENS, pr.ST_Q_LENS, causal), lse64, smax
    return torch.tensor(np.nan_to_num(o64)).to(DEV), lse64, smax


@pytest.mark.parametrize("causal", [True, False], ids=["causal", "full"])
@pytest.mark.parametrize("d", [128, 64])
@pytest.mark.parametrize("dtype", dr.DTYPES)
@pytest.mark.parametrize("pattern", list(pr.ST_PATTERNS))
def test_staircase_contiguous(pattern, dtype, d, causal):
    """Every staircase pattern on the contiguous 16-bit cache: O and LSE against
    the references at the project's gates."""
    tq, tk, tv = _st(pattern, d, "q", dtype)[:3]
    out, lse = prefill(tq, tk, tv, _lens(pr.ST_KV_LENS), _lens(pr.ST_Q_LENS), causal=causal, return_lse=True,
                       out=dr.nan_fill(torch.empty_like(tq)))
    pr.check(out, lse, _st_refs(pattern, d, "q", causal, dtype is F16), pr.ST_Q_LENS, dtype,
             f"staircase {pattern} {dr.name(dtype)} d={d} causal={causal}")
    for bi, n in enumerate(pr.ST_Q_LENS):  # rows past n_b: not written
        assert _nan_bits(out[bi, :, n:]), bi


@pytest.mark.parametrize("d", [128, 64])
@pytest.mark.parametrize("dtype", dr.DTYPES)
@pytest.mark.parametrize("pattern", ["asc4.5", "over8", "jump"])
def test_staircase_other_cache_forms(pattern, dtype, d):
    """delta in Q and unit scales: paged (page sizes 64 and 128) bit-equal to
    contiguous, the FP8 entries bit-equal to the 16-bit entry on the same
    values.  delta carried by a non-power-of-two k_scale, beside a
    non-power-of-two v_scale: the FP8 entry against contract_f64 on the
    dequantised cache, paged FP8 bit-equal to it."""
    tl, ql = _lens(pr.ST_KV_LENS), _lens(pr.ST_Q_LENS)
    for causal in (True, False):
        what = f"staircase {pattern} {dr.name(dtype)} d={d} causal={causal}"
        kw = dict(causal=causal, return_lse=True)
        tq, tk, tv, k8, v8, ksc, vsc = _st(pattern, d, "q", dtype)
        want = prefill(tq, tk, tv, tl, ql, **kw)
        pr.check(*want, _st_refs(pattern, d, "q", causal, dtype is F16), pr.ST_Q_LENS, dtype, what + " contig")
        for ps in (64, 128):
            kp, vp, table = _paginate(tk, tv, ps, pr.ST_KV_LENS, seed=ps, filler="junk")
            assert _same_rows(prefill_paged(tq, kp, vp, table, tl, ql, **kw), want, pr.ST_Q_LENS), (what, ps)
        assert _same_rows(prefill(tq, k8, v8, tl, ql, k_scale=ksc, v_scale=vsc, **kw), want, pr.ST_Q_LENS), what
        kp, vp, table = _paginate(k8, v8, 128, pr.ST_KV_LENS, seed=5, filler="junk")
        got = prefill_paged(tq, kp, vp, table, tl, ql, k_scale=ksc, v_scale=vsc, **kw)
        assert _same_rows(got, want, pr.ST_Q_LENS), what

        tq, _, _, k8, v8, ksc, vsc = _st(pattern, d, "scale", dtype)
        want = prefill(tq, k8, v8, tl, ql, k_scale=ksc, v_scale=vsc, **kw)
        pr.check(*want, _st_refs(pattern, d, "scale", causal, False), pr.ST_Q_LENS, dtype, what + " kv8 scales")
        for ps in (64, 128):
            kp, vp, table = _paginate(k8, v8, ps, pr.ST_KV_LENS, seed=ps + 1, filler="junk")
            got = prefill_paged(tq, kp, vp, table, tl, ql, k_scale=ksc, v_scale=vsc, **kw)
            assert _same_rows(got, want, pr.ST_Q_LENS), (what, ps)


@pytest.mark.parametrize("d", [128, 64])
@pytest.mark.parametrize("dtype", dr.DTYPES)
@pytest.mark.parametrize("pattern", ["asc4.5", "over8"])
def test_staircase_packed_twins(pattern, dtype, d):
    """The same inputs through the packed entries: rows of each sequence bit for
    bit those of the padded result, in all four cache forms (the FP8 ones with
    delta carried by k_scale)."""
    n = pr.ST_Q_LENS
    cu, total = vr.cu_of(n), sum(n) + 12  # a tail of rows that belong to no sequence
    tl, ql, tcu = _lens(pr.ST_KV_LENS), _lens(n), _lens(cu)
    for causal in (True, False):
        kw = dict(causal=causal, return_lse=True)
        for form in ("contig", "paged", "contig_kv8", "paged_kv8"):
            kv8 = form.endswith("kv8")
            tq, tk, tv, k8, v8, ksc, vsc = _st(pattern, d, "scale" if kv8 else "q", dtype)
            k, v = (k8, v8) if kv8 else (tk, tv)
            sc = dict(k_scale=ksc, v_scale=vsc) if kv8 else {}
            qp = vr.pack(tq, n, total=total, fill=dr.NAN_BITS)
            if form.startswith("paged"):
                kp, vp, table = _paginate(k, v, 64, pr.ST_KV_LENS, seed=7, filler="junk")
                got = prefill_varlen_paged(qp, kp, vp, table, tcu, tl, **kw, **sc)
                want = prefill_paged(tq, kp, vp, table, tl, ql, **kw, **sc)
            else:
                got = prefill_varlen(qp, k, v, tcu, tl, **kw, **sc)
                want = prefill(tq, k, v, tl, ql, **kw, **sc)
            got = (vr.unpack(got[0], cu, pr.ST_SQ), vr.unpack(got[1], cu, pr.ST_SQ, fill=float("-inf")))
            assert _same_rows(got, want, n), (pattern, dr.name(dtype), d, causal, form)
            assert bool(torch.isfinite(got[0]).all())


@pytest.mark.parametrize("sq", [1, 16])
@pytest.mark.parametrize("dtype", dr.DTYPES)
def test_staircase_agrees_with_decode(dtype, sq):
    """q_lens None and Sq <= 16 on the just-over-8 pattern: within the sum of the
    two gates of decode (the tolerance of test_prefill_gpu's
    test_agrees_with_decode), on all four forms."""
    b, hq, hkv, cap, d = 3, 8, 2, 384, 128
    kv_lens = (70, 300, 384)
    tl = _lens(kv_lens)
    gate = 2 * (dr.GATE_F16 if dtype is F16 else dr.GATE_BF16)
    shape = dict(b=b, hq=hq, hkv=hkv, sq=sq, cap=cap, kv_lens=kv_lens)
    for carry in ("q", "scale"):
        st = pr.staircase("over8", d, carry, **shape)
        smax = pr.contract_f64(st.q, *st.dequant(), kv_lens, None, True, with_smax=True)[3]
        tq = torch.tensor(st.q).to(dtype).to(DEV)
        k8, v8 = (_pad(torch.tensor(a).float().to(FP8).to(DEV), kv_lens) for a in (st.k, st.v))
        sc = dict(k_scale=_scale_t(st.k_scale), v_scale=_scale_t(st.v_scale))
        kp8, vp8, table8 = _paginate(k8, v8, 128, kv_lens, seed=2)
        pairs = {
            "contig_kv8": (prefill(tq, k8, v8, tl, return_lse=True, **sc),
                           decode(tq, k8, v8, tl, return_lse=True, **sc)),
            "paged_kv8": (prefill_paged(tq, kp8, vp8, table8, tl, return_lse=True, **sc),
                          decode_paged(tq, kp8, vp8, table8, tl, return_lse=True, **sc)),
        }
        if carry == "q":
            tk, tv = (_pad(torch.tensor(a).to(dtype).to(DEV), kv_lens) for a in (st.k, st.v))
            kp, vp, table = _paginate(tk, tv, 128, kv_lens, seed=2)
            pairs["contig"] = (prefill(tq, tk, tv, tl, return_lse=True), decode(tq, tk, tv, tl, return_lse=True))
            pairs["paged"] = (prefill_paged(tq, kp, vp, table, tl, return_lse=True),
                              decode_paged(tq, kp, vp, table, tl, return_lse=True))
        for form, ((o1, l1), (o2, l2)) in pairs.items():
            err = float((o1.float() - o2.float()).abs().max())
            print(f"{form} {carry} {dr.name(dtype)} Sq={sq}: |prefill - decode| O {err:.3e}")
            assert bool(torch.isfinite(o1).all()) and err <= gate, (form, carry, err)
            assert torch.equal(torch.isneginf(l1), torch.isneginf(l2)), (form, carry)
            fin = torch.isfinite(l2)
            assert float((l1[fin] - l2[fin]).abs().max()) <= 2 * (2.0 ** -10 * smax + 1e-5), (form, carry)


# ---- 2. the random Q, K x 4 case the other tiers have -------------------------------------

@pytest.mark.parametrize("form", ["contig", "paged_kv8"])
@pytest.mark.parametrize("d", [128, 64])
@pytest.mark.parametrize("dtype", dr.DTYPES)
def test_peaked_random(dtype, d, form):
    """decode_refs.inputs with Q and K times 4 (exact in 16 bits): scores 16 times
    as wide, as test_peaked_softmax of decode and the forward tiers' peaked
    tests have them."""
    b, hq, hkv, sq, cap = 2, 4, 2, 321, 640
    q_lens, kv_lens = (321, 290), (321, 200 + 290)
    q, k, v = dr.inputs(b, hq, hkv, sq, cap, d)
    tq, tk, tv = dr.dev(q).to(dtype) * 4, dr.dev(k).to(dtype) * 4, dr.dev(v).to(dtype)
    assert torch.equal(tq.float(), dr.dev(q).to(dtype).float() * 4)
    tl, ql = _lens(kv_lens), _lens(q_lens)
    for causal in (True, False):
        what = f"peaked {form} {dr.name(dtype)} d={d} causal={causal}"
        if form == "contig":
            refs = _refs(tq, tk, tv, kv_lens, q_lens, causal, dtype is F16)
            out, lse = prefill(tq, _pad(tk, kv_lens), _pad(tv, kv_lens), tl, ql, causal=causal, return_lse=True)
        else:
            ks_, vs_ = _scale_t(K_SCALE)[None, :, None, None], _scale_t(V_SCALE)[None, :, None, None]
            k8, v8 = (tk.float() / ks_).to(FP8), (tv.float() / vs_).to(FP8)
            kd, vd = k8.float() * ks_, v8.float() * vs_
            assert bool(torch.isfinite(kd).all()) and bool(torch.isfinite(vd).all())
            for x in (kd, vd):  # power-of-two scales: exact in both 16-bit types, so the oracle applies
                assert torch.equal(x.to(dtype).float(), x)
            refs = _refs(tq, kd.to(dtype), vd.to(dtype), kv_lens, q_lens, causal, dtype is F16)
            kp, vp, table = _paginate(_pad(k8, kv_lens), _pad(v8, kv_lens), 128, kv_lens, seed=4, filler="junk")
            out, lse = prefill_paged(tq, kp, vp, table, tl, ql, causal=causal, return_lse=True,
                                     k_scale=_scale_t(K_SCALE), v_scale=_scale_t(V_SCALE))
        pr.check(out, lse, refs, q_lens, dtype, what)


# ---- 3. offsets past 4 GiB ----------------------------------------------------------------

def _free():
    torch.cuda.empty_cache()


def _rand_v(shape, dtype, seed):
    """V in [-0.5, 0.5) as the suite's own inputs have it, so |O| < 0.5 under the absolute gates."""
    return dr.rand(shape, dtype, seed) * 0.5


def _bytes(t):
    """t as uint8 (FP8 tensors are copied and indexed through this view)."""
    return t.view(torch.uint8)


def _quant_heads(x, scales):
    """E4M3 codes of x [.., Hkv, rows, D] under one fp32 scale per K/V head, and
    what they dequantise to in float64: float64(code) * float64(scale)."""
    s = scales[:, None, None]
    codes = (x.float() / s).to(FP8)
    deq = codes.float().double() * s.double()
    assert bool(torch.isfinite(deq).all())
    return codes, deq


def _live_refs(tq, kd, vd, kv_lens, q_lens, dtype, oracle=True):
    return _refs(tq, kd, vd, kv_lens, q_lens, True, oracle and dtype is F16)


@pytest.mark.parametrize("kv8", [False, True], ids=["16bit", "kv8"])
@pytest.mark.parametrize("dtype", dr.DTYPES)
def test_prefill_cache_past_4gib(dtype, kv8):
    """Contiguous K and V above 4 GiB each: all lengths zero but the first and
    the last element's, whose head offsets (the last: past 2^32 bytes) a 32-bit
    product would wrap.  The other elements' O rows keep their NaN pre-fill."""
    b, hq, hkv, cap, d, sq = (34 if kv8 else 17), 16, 8, 131072 + 8, 128, 130
    assert b * hkv * cap * d * (1 if kv8 else 2) > 4 << 30 and (b - 1) * hkv * cap * d * (1 if kv8 else 2) > 4 << 30
    live, keys = (0, b - 1), 256
    kv_lens = [0] * b
    q_lens = [0] * b
    kv_lens[0], kv_lens[-1], q_lens[0], q_lens[-1] = 200, 213, sq, sq - 1
    tq = dr.rand((b, hq, sq, d), dtype, 1)
    small = [dr.rand((2, hkv, keys, d), dtype, 2), _rand_v((2, hkv, keys, d), dtype, 3)]
    sc, deq = {}, small
    if kv8:
        sc = dict(k_scale=_scale_t(A_SCALES[0]), v_scale=_scale_t(A_SCALES[1]))
        small, deq = zip(*(_quant_heads(x, s) for x, s in zip(small, sc.values())))
    k = torch.empty((b, hkv, cap, d), dtype=small[0].dtype, device=DEV)
    v = torch.empty_like(k)
    for big, part in zip((k, v), small):
        _bytes(big)[0, :, :keys], _bytes(big)[-1, :, :keys] = _bytes(part)[0], _bytes(part)[1]
    out = dr.nan_fill(torch.empty_like(tq))
    got, lse = prefill(tq, k, v, _lens(kv_lens), _lens(q_lens), out=out, return_lse=True, **sc)
    assert got is out
    two = lambda t: t[list(live)]  # noqa: E731
    refs = _live_refs(two(tq), deq[0], deq[1], [kv_lens[i] for i in live], [q_lens[i] for i in live], dtype,
                      oracle=not kv8)
    pr.check(two(out), two(lse), refs, (sq, sq - 1), dtype, f"cache past 4 GiB {dr.name(dtype)} kv8={kv8}")
    assert _nan_bits(out[1:-1]) and _nan_bits(out[-1, :, sq - 1:])
    del k, v, big
    _free()


@pytest.mark.parametrize("kv8", [False, True], ids=["16bit", "kv8"])
@pytest.mark.parametrize("dtype", dr.DTYPES)
def test_prefill_pool_past_4gib(dtype, kv8):
    """A page pool above 4 GiB in bytes and above 2^31 in elements; both
    sequences' tables interleave the pool's last pages with its first.  Bit-equal
    to the contiguous entry on the gathered cache, and within the gates of
    the reference."""
    hq, hkv, ps, d, sq = 8, 8, 128, 128, 130
    num_pages = 33000 if kv8 else 16500
    assert num_pages * hkv * ps * d > 1 << 31 and num_pages * hkv * ps * d * (1 if kv8 else 2) > 4 << 30
    table = torch.tensor([[num_pages - 1, 0, num_pages - 3], [1, num_pages - 2, 2]], dtype=torch.int32, device=DEV)
    kv_lens, q_lens = (330, 260), (sq, sq - 3)
    sc = dict(k_scale=_scale_t(A_SCALES[0]), v_scale=_scale_t(A_SCALES[1])) if kv8 else {}
    pools = []
    for i, s in enumerate((2, 3)):
        pool = torch.empty((num_pages, hkv, ps, d), dtype=FP8 if kv8 else dtype, device=DEV)
        data = (dr.rand, _rand_v)[i]((6, hkv, ps, d), dtype, s)
        if kv8:
            data = _quant_heads(data, list(sc.values())[i])[0]
        _bytes(pool)[table.flatten().long()] = _bytes(data)
        pools.append(pool)
    tq = dr.rand((2, hq, sq, d), dtype, 1)
    tl, ql = _lens(kv_lens), _lens(q_lens)
    got = prefill_paged(tq, pools[0], pools[1], table, tl, ql, return_lse=True, out=torch.zeros_like(tq), **sc)
    gk, gv = (dr.gather(_bytes(p), table).view(p.dtype) for p in pools)
    want = prefill(tq, gk, gv, tl, ql, return_lse=True, out=torch.zeros_like(tq), **sc)
    assert _same_rows(got, want, q_lens)
    if kv8:
        gk = gk.float().double() * sc["k_scale"].double()[None, :, None, None]
        gv = gv.float().double() * sc["v_scale"].double()[None, :, None, None]
    pr.check(*got, _live_refs(tq, gk, gv, kv_lens, q_lens, dtype, oracle=not kv8), q_lens, dtype,
             f"pool past 4 GiB {dr.name(dtype)} kv8={kv8}")
    del pools, pool
    _free()


@pytest.mark.parametrize("dtype", dr.DTYPES)
def test_prefill_q_and_o_past_4gib_padded(dtype):
    """Q and O [B, Hq, Sq, D] above 4 GiB each; q_lens zero but for the first and
    the last element, whose row offsets (the last head's: past 2^32 bytes) a
    32-bit product would wrap.  Everything but their rows keeps its pre-fill."""
    b, hq, hkv, sq, d, cap, n = 5, 2, 1, 1_900_000, 128, 256, 130
    row = 2 * d
    assert b * hq * sq * row > 4 << 30 and (b * hq - 1) * sq * row > 4 << 30
    q_lens, kv_lens = [n, 0, 0, 0, n - 1], [180, 0, 0, 0, 170]
    tk, tv = dr.rand((b, hkv, cap, d), dtype, 2), _rand_v((b, hkv, cap, d), dtype, 3)
    tq = torch.empty((b, hq, sq, d), dtype=dtype, device=DEV)
    live = dr.rand((2, hq, n, d), dtype, 1)
    tq[0, :, :n], tq[-1, :, :n] = live[0], live[1]
    out = dr.nan_fill(torch.empty_like(tq))
    got, lse = prefill(tq, tk, tv, _lens(kv_lens), _lens(q_lens), out=out, return_lse=True)
    o2 = torch.stack((out[0, :, :n], out[-1, :, :n]))
    l2 = torch.stack((lse[0, :, :n], lse[-1, :, :n]))
    refs = _live_refs(live, tk[[0, -1]], tv[[0, -1]], [180, 170], [n, n - 1], dtype)
    pr.check(o2, l2, refs, (n, n - 1), dtype, f"Q/O past 4 GiB padded {dr.name(dtype)}")
    # the rows next to the live ones, the dead elements' first and last rows, and the
    # rows 2^32 bytes below the last head's (where a wrapped offset would have written)
    wrapped = ((b * hq - 1) * sq * row - WRAP) // row
    flat = out.view(-1, d)
    assert _nan_bits(out[0, :, n:n + 4096]) and _nan_bits(out[-1, :, n - 1:n + 4096])
    assert _nan_bits(out[1:-1, :, :4096]) and _nan_bits(out[:, :, -4096:])
    assert _nan_bits(flat[wrapped - 64:wrapped + n + 64])
    del tq, out, flat, got
    _free()


@pytest.mark.parametrize("dtype", dr.DTYPES)
def test_prefill_q_and_o_past_4gib_packed(dtype):
    """Packed Q and O [T, Hq, D] above 4 GiB each with cu_seqlens = [T - 200,
    T - 70, T]: a leading range that belongs to no sequence, the live rows past
    2^32 bytes."""
    total, hq, hkv, d, cap = 9_500_000, 2, 1, 128, 256
    row = 2 * d
    assert (total - 200) * hq * row > 4 << 30
    cu, n, kv_lens = [total - 200, total - 70, total], (130, 70), (180, 170)
    tk, tv = dr.rand((2, hkv, cap, d), dtype, 2), _rand_v((2, hkv, cap, d), dtype, 3)
    live = dr.rand((2, hq, 130, d), dtype, 1)
    qp = torch.empty((total, hq, d), dtype=dtype, device=DEV)
    qp[total - 200:] = vr.pack(live, n)
    out = dr.nan_fill(torch.empty_like(qp))
    got, lse = prefill_varlen(qp, tk, tv, _lens(cu), _lens(kv_lens), out=out, return_lse=True)
    assert got is out and lse.shape == (hq, total)
    local = [0, 130, 200]
    o2 = vr.unpack(out[total - 200:], local, 130)
    l2 = vr.unpack(lse[:, total - 200:].contiguous(), local, 130, fill=float("-inf"))
    pr.check(o2, l2, _live_refs(live, tk, tv, kv_lens, n, dtype), n, dtype, f"Q/O past 4 GiB packed {dr.name(dtype)}")
    wrapped = ((total - 200) * hq * row - WRAP) // (hq * row)
    assert _nan_bits(out[:4096]) and _nan_bits(out[total - 200 - 4096:total - 200])
    assert _nan_bits(out[wrapped - 64:wrapped + 200 + 64])
    # and the padded entry on the unpacked rows gives the same bits
    want = prefill(live, tk, tv, _lens(kv_lens), _lens(n), return_lse=True)
    assert _same_rows((o2, l2), want, n)
    del qp, out, got
    _free()


# ---- append ------------------------------------------------------------------------------

SENTINEL = 0xA5


def _expected_bytes(x, kv8, scales):
    """uint8 [.., Hkv, n, row bytes] the cache must hold for the source rows x
    [.., Hkv, n, D]: the source's own bits, or the E4M3 contract's bytes
    (tests/fp8_contract.py) under each head's scale."""
    xc = x.cpu()
    if not kv8:
        return xc.view(torch.uint8)
    heads = [fp8_contract.torch_reference_bytes(xc[..., h, :, :], scales[h]) for h in range(xc.shape[-3])]
    return torch.stack(heads, dim=-3)


class _Rows:
    """The cache rows (flat indices into [rows, row bytes] views of K and V) an
    append must write, with the bytes expected there, and the sentinel rows it
    must leave alone: the two rows before and after every written run and the
    rows 2^32 bytes below the written ones."""

    def __init__(self, caches, crow):
        self.flat = [c.view(torch.uint8).view(-1, crow) for c in caches]
        self.crow, self.idx, self.want = crow, [], ([], [])

    def run(self, first, want_k, want_v):
        self.idx.append(torch.arange(first, first + want_k.shape[0]))
        self.want[0].append(want_k)
        self.want[1].append(want_v)

    def arm(self):
        idx = torch.cat(self.idx)
        assert len(torch.unique(idx)) == len(idx) and int(idx.max()) * self.crow > WRAP
        edges = torch.cat([torch.cat((r[:1] - 2, r[:1] - 1, r[-1:] + 1, r[-1:] + 2)) for r in self.idx])
        guard = torch.cat((edges, idx - WRAP // self.crow))
        guard = guard[(guard >= 0) & (guard < self.flat[0].shape[0])]
        self.guard = guard[~torch.isin(guard, idx)].to(DEV)
        assert int((self.guard + WRAP // self.crow)[:, None].eq(idx.to(DEV)[None, :]).sum()) > 0  # wrapped rows are in
        self.rows = idx.to(DEV)
        for f in self.flat:
            f[self.guard] = SENTINEL
            f[self.rows] = SENTINEL ^ 0xff

    def check(self, what):
        for f, want, name in zip(self.flat, self.want, "KV"):
            assert torch.equal(f[self.rows].cpu(), torch.cat(want)), (what, name)
            assert bool((f[self.guard] == SENTINEL).all()), (what, name, "a row next to or 2^32 below a written one")


APPEND_FORMS = ["contig", "paged", "contig_kv8", "paged_kv8"]


@pytest.mark.parametrize("packed", [False, True], ids=["padded", "packed"])
@pytest.mark.parametrize("form", APPEND_FORMS)
def test_append_past_4gib(form, packed):
    """Destination rows past 4 GiB (the last element's heads, or the pool's last
    pages) beside rows at the start: the written rows hold the expected bytes,
    the rows around every run and those 2^32 bytes below keep a sentinel, and
    prefill over the appended cache is within the gates."""
    kv8, paged = form.endswith("kv8"), form.startswith("paged")
    dtype = BF16 if packed else F16
    hkv, hq, d, sn = 8, 8, 128, 150
    crow = d if kv8 else 2 * d
    cdtype = FP8 if kv8 else dtype
    scales = A_SCALES if kv8 else (None, None)
    sc = dict(k_scale=_scale_t(scales[0]), v_scale=_scale_t(scales[1])) if kv8 else {}
    if paged:
        ps, num_pages = 128, 33000 if kv8 else 16500
        assert num_pages * hkv * ps * crow > 4 << 30
        b, n = 2, (150, 140)
        pages = [[0, num_pages - 2], [num_pages - 1, 1]]
        table = torch.tensor(pages, dtype=torch.int32, device=DEV)
        caches = [torch.empty((num_pages, hkv, ps, d), dtype=cdtype, device=DEV) for _ in range(2)]
    else:
        b, cap = (34 if kv8 else 17), 131072 + 8
        assert (b - 1) * hkv * cap * crow > 4 << 30
        n = (40,) + (0,) * (b - 2) + (33,)
        caches = [torch.empty((b, hkv, cap, d), dtype=cdtype, device=DEV) for _ in range(2)]
    live = [bi for bi in range(b) if n[bi]]
    knew, vnew = dr.rand((b, hkv, sn, d), dtype, 11), _rand_v((b, hkv, sn, d), dtype, 12)
    want = [_expected_bytes(x, kv8, s) for x, s in zip((knew, vnew), scales)]  # [B, Hkv, Sn, crow]
    rows = _Rows(caches, crow)
    for bi in live:
        for hk in range(hkv):
            if paged:
                for j, pg in enumerate(pages[bi]):
                    t0, t1 = j * ps, min(n[bi], (j + 1) * ps)
                    rows.run((pg * hkv + hk) * ps, want[0][bi, hk, t0:t1], want[1][bi, hk, t0:t1])
            else:
                rows.run((bi * hkv + hk) * cap, want[0][bi, hk, :n[bi]], want[1][bi, hk, :n[bi]])
    rows.arm()
    tl = _lens(n)  # the lengths after the append: every prompt starts at row 0
    if packed:
        cu = _lens(vr.cu_of(n))
        kp_, vp_ = vr.pack(knew, n), vr.pack(vnew, n)
        if paged:
            append_varlen_paged(kp_, vp_, *caches, table, cu, tl, **sc)
        else:
            append_varlen(kp_, vp_, *caches, cu, tl, **sc)
    elif paged:
        append_paged(knew, vnew, *caches, table, tl, _lens(n), **sc)
    else:
        append(knew, vnew, *caches, tl, _lens(n), **sc)
    torch.cuda.synchronize()
    rows.check(f"append {form} packed={packed}")

    # the chain: prefill over what was appended, the whole prompt as the chunk
    tq = dr.rand((b, hq, sn, d), dtype, 13)
    if paged:
        got = prefill_paged(tq, *caches, table, tl, _lens(n), return_lse=True, **sc)
    else:
        got = prefill(tq, *caches, tl, _lens(n), return_lse=True, **sc)
    if kv8:
        kd, vd = (w.view(FP8).float().double() * torch.tensor(s, dtype=torch.float32).double()[None, :, None, None]
                  for w, s in zip(want, scales))
    else:
        kd, vd = knew.cpu(), vnew.cpu()
    two = lambda t: t[live]  # noqa: E731
    refs = _live_refs(two(tq), two(kd), two(vd), [n[bi] for bi in live], [n[bi] for bi in live], dtype,
                      oracle=not kv8)
    pr.check(two(got[0]), two(got[1]), refs, [n[bi] for bi in live], dtype, f"append -> prefill {form} packed={packed}")
    del caches, rows
    _free()


def test_append_packed_source_past_4gib():
    """The packed source k_new / v_new [T, Hkv, D] above 4 GiB each, the live
    tokens at its end (cu_seqlens = [T - 200, T - 70, T]): a 32-bit source
    offset would copy other rows."""
    total, hkv, d, cap = 2_200_000, 8, 128, 256
    assert (total - 200) * hkv * 2 * d > 4 << 30
    n, prefix = (130, 70), (50, 100)
    kv_lens = [p + x for p, x in zip(prefix, n)]
    cu = [total - 200, total - 70, total]
    src = [dr.rand((200, hkv, d), F16, s) for s in (11, 12)]
    news = []
    for s in src:
        big = torch.empty((total, hkv, d), dtype=F16, device=DEV)
        big[total - 200:] = s
        # the rows a wrapped source offset would read instead
        big.view(-1, d)[((total - 200) * hkv * 2 * d - WRAP) // (2 * d):][:200 * hkv].fill_(3.0)
        news.append(big)
    caches = [torch.full((2, hkv, cap, d), 2.0, dtype=F16, device=DEV) for _ in range(2)]
    append_varlen(*news, *caches, _lens(cu), _lens(kv_lens))
    torch.cuda.synchronize()
    for c, s in zip(caches, src):
        want = torch.full_like(c, 2.0)
        want[0, :, prefix[0]:kv_lens[0]] = s[:130].permute(1, 0, 2)
        want[1, :, prefix[1]:kv_lens[1]] = s[130:].permute(1, 0, 2)
        assert torch.equal(c, want)
    del news, big
    _free()
