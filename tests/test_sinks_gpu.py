"""GPU tests of attention sinks: the fa_decode_sink_*, fa_prefill_sink_* and
fa_prefill_varlen_sink_* entries through the `sinks=` keyword of the six Python
functions and through ctypes, over the four cache forms.

References, gates and the closed-form inputs are tests/sink_refs.py's (the
project's: census at keysense_inputs' gates, fp16 O 1e-3 against the CPU-oracle
rows carried over by O = O0 sigmoid(LSE0 - sink), bf16 O 5e-3 against fp32
torch with an explicit extra softmax column, LSE 2^-10 max|scaled score or
sink| + 1e-5); tests/test_sinks_cpu.py holds them against a float64 restatement
at half of each gate.  Paged results are held to the contiguous one BIT FOR BIT
and FP8 at unit scales to 16-bit on values exact in E4M3, so every check made
on the contiguous result is made on all four forms.

Census: every score is s and sinks[h] = s + ln(m_h), m_h = 1 + 2 h, so head h's
sink weighs as m_h more keys: O = count / (n + m_h), LSE = s + log(n + m_h).  A
sink taken from another head, counted twice or dropped moves a denominator by
>= 1 / (n + m_max + 1); test_sinks_cpu.py asserts n + m_max <= 250 where a
window or a length cuts at the shapes used here.
"""
import functools

import numpy as np
import pytest
import torch

import decode_refs as dr
import fa_mi355x
import prefill_refs as pr
import sink_refs as sr
import varlen_refs as vr
import window_refs as wr

pytestmark = pytest.mark.gpu

DEV = "cuda"
FP8 = torch.float8_e4m3fn
PAD8 = 0x7f  # the E4M3 NaN
F16, BF16 = torch.float16, torch.bfloat16
NINF = float("-inf")
K_SCALE = (2.0 ** -6, 2.0 ** -3)
V_SCALE = (2.0 ** -4, 2.0 ** -8)
LEVELS = ((0.0, 0.0), (4.0, -4.0))  # (Q, K): every score 0, or -181.02 at D = 128 (-128 at D = 64)

prefill = fa_mi355x.flash_attention_prefill
prefill_paged = fa_mi355x.flash_attention_prefill_paged
prefill_varlen = fa_mi355x.flash_attention_prefill_varlen
prefill_varlen_paged = fa_mi355x.flash_attention_prefill_varlen_paged
decode = fa_mi355x.flash_attention_decode
decode_paged = fa_mi355x.flash_attention_decode_paged


def _lens(vals):
    return None if vals is None else dr.lens(vals)


def _dev32(x):
    return None if x is None else torch.as_tensor(x, dtype=torch.float32).to(DEV).contiguous()


def _nan_rows(rows):
    if rows.element_size() == 1:
        rows.view(torch.uint8).fill_(PAD8)
    else:
        rows.view(torch.int16).fill_(dr.NAN_BITS)


def _pad(t, lens, cap_to=None):
    """A copy with NaN bits (the E4M3 NaN in an FP8 cache) in the rows at or past
    each length, the capacity grown to `cap_to` rows of the same."""
    if cap_to is not None and cap_to > t.shape[2]:
        big = torch.empty(t.shape[:2] + (cap_to,) + t.shape[3:], dtype=t.dtype, device=t.device)
        big[:, :, :t.shape[2]] = t
        t = big
    else:
        t = t.clone()
    for i, n in enumerate(lens):
        _nan_rows(t[i, :, min(int(n), t.shape[2]):])
    return t


def _paginate(k, v, page_size, lens, **kw):
    cap = -(-k.shape[2] // page_size) * page_size
    k, v = _pad(k, lens, cap), _pad(v, lens, cap)
    one = k.dtype is FP8
    if one:
        k, v = k.view(torch.uint8), v.view(torch.uint8)
    kp, vp, table = dr.paginate(k, v, page_size, lens, **kw)
    return (kp.view(FP8), vp.view(FP8), table) if one else (kp, vp, table)


def _cache_form(form, k, v, scales):
    """(k, v, scale kwargs) of a cache form from the clean 16-bit caches: a kv8
    form with scales=None reads their exact E4M3 conversion at unit scales,
    otherwise scales = (k8, v8, k_scale, v_scale)."""
    if not form.endswith("kv8"):
        return k, v, {}
    if scales is None:
        k8, v8 = k.to(FP8), v.to(FP8)
        assert torch.equal(k8.to(k.dtype), k) and torch.equal(v8.to(v.dtype), v)
        return k8, v8, {}
    return scales[0], scales[1], dict(k_scale=scales[2], v_scale=scales[3])


def _prefill_form(form, ps, q, k, v, kv_lens, q_lens, window, sinks, scales=None, causal=True, seed=1):
    k, v, sc = _cache_form(form, k, v, scales)
    tl, ql = _lens(kv_lens), _lens(q_lens)
    lens = kv_lens if kv_lens is not None else [k.shape[2]] * k.shape[0]
    if form.startswith("paged"):
        kp, vp, table = _paginate(k, v, ps, lens, seed=seed + ps)
        return prefill_paged(q, kp, vp, table, tl, ql, causal=causal, return_lse=True, window=window, sinks=sinks,
                             **sc)
    return prefill(q, _pad(k, lens), _pad(v, lens), tl, ql, causal=causal, return_lse=True, window=window,
                   sinks=sinks, **sc)


def _decode_form(form, ps, q, k, v, lens, window, ns, sinks, scales=None, causal=True):
    k, v, sc = _cache_form(form, k, v, scales)
    tl = _lens(lens)
    if form.startswith("paged"):
        kp, vp, table = _paginate(k, v, ps, lens, seed=2 + ps)
        return decode_paged(q, kp, vp, table, tl, causal=causal, return_lse=True, num_splits=ns, window=window,
                            sinks=sinks, **sc)
    return decode(q, _pad(k, lens), _pad(v, lens), tl, causal=causal, return_lse=True, num_splits=ns,
                  window=window, sinks=sinks, **sc)


def _same_rows(a, b, n):
    return all(torch.equal(a[0][bi, :, :nb], b[0][bi, :, :nb]) and torch.equal(a[1][bi, :, :nb], b[1][bi, :, :nb])
               for bi, nb in enumerate(n))


def _interval_t(kv_lens, q_lens, b, sq, cap, window):
    lo, hi = wr.interval(kv_lens, q_lens, b, sq, cap, window)
    return torch.from_numpy(lo)[:, None, :], torch.from_numpy(hi)[:, None, :]


# ---- 1. census with per-head sinks ------------------------------------------------------

B, HQ, HKV, SQ, CAP = pr.KS_B, 4, 2, pr.KS_SQ, pr.KS_CAP
Q_LENS, KV_LENS = pr.KS_Q_LENS, pr.KS_KV_LENS
PFORMS = [("paged", 64), ("paged", 256), ("contig_kv8", 0), ("paged_kv8", 64), ("paged_kv8", 256)]


def _check_prefill_census(o, lse, counts, kv_lens, q_lens, cap, window, score, m, what):
    b, _, sq, _ = o.shape
    lo, hi = _interval_t(kv_lens, q_lens, b, sq, cap, window)
    for bi, n in enumerate(pr.n_rows(q_lens, b, sq)):
        if n:
            sr.check_census(o[bi, :, :n], lo[bi, :, :n], hi[bi, :, :n], counts, score, m, f"{what} b={bi}",
                            lse=lse[bi, :, :n]).require()


# (D, (Q, K)): s = 0 at both head dims, s = -181.02 at D = 128
PRE_LEVELS = [pytest.param(128, LEVELS[0], id="d128-s0"), pytest.param(128, LEVELS[1], id="d128-s181"),
              pytest.param(64, LEVELS[0], id="d64-s0")]


@pytest.mark.parametrize("window", [0, 40, 128, 130])
@pytest.mark.parametrize("d,level", PRE_LEVELS)
@pytest.mark.parametrize("dtype", dr.DTYPES)
def test_prefill_census_with_per_head_sinks(dtype, d, level, window):
    """Hq = 4 over Hkv = 2, Sq 321 / 290 behind a 200-key prefix (three query
    blocks): each head's denominator holds its own sink once.  Paged (pages of 64
    and 256) equals contiguous bit for bit, FP8 at unit scales equals 16-bit.

    The fp16 cases at s = -181.02 hold the O gate only because a head with a
    sink scales its scores in fp32: fp16's rounded Q * log2(e)/sqrt(D) puts
    every score of these inputs 0.066 low, which cancels in O without a sink
    and moved O by 0.065 m / (n + m) beside one (2.6e-3 to 1.0e-2 measured
    before the kernel did so)."""
    qval, kval = level
    score = wr.census_score(qval, kval, d)
    sinks, m = sr.census_sinks(HQ, score)
    q, k, v, counts = wr.census_qkv((B, HQ, SQ, d), (B, HKV, CAP, d), qval, kval, "stripe", dtype, DEV)
    base = _prefill_form("contig", 0, q, k, v, KV_LENS, Q_LENS, window, _dev32(sinks))
    what = f"census {dr.name(dtype)} d={d} W={window} s={score:.2f}"
    for form, ps in PFORMS:
        got = _prefill_form(form, ps, q, k, v, KV_LENS, Q_LENS, window, _dev32(sinks))
        assert _same_rows(got, base, Q_LENS), f"{what} {form} page={ps}"
    _check_prefill_census(*base, counts, KV_LENS, Q_LENS, CAP, window, score, m, what)


DB, DCAP = 3, 1024
DLENS = (1, 130, 1000)
SPLITS = (1, 3, 8, 0)  # 8 over a 1-tile window: pieces with an empty range, and the sink still counts once
# (Hq, Hkv, Sq): a head change inside a 16-row block (group 3); 128 rows, two row groups
GEOMS = [(6, 2, 1), (6, 2, 4), (6, 2, 16), (16, 2, 16)]


@pytest.mark.parametrize("window", [0, 5, 64, 100])
@pytest.mark.parametrize("hq,hkv,sq", GEOMS, ids=[f"hq{a}_sq{c}" for a, _, c in GEOMS])
@pytest.mark.parametrize("dtype", dr.DTYPES)
def test_decode_census_with_per_head_sinks(dtype, hq, hkv, sq, window):
    """Row r of a K/V head's group * Sq rows belongs to head hkv * group + r / Sq:
    each row's denominator holds its own head's sink exactly once, unsplit (the
    in-CU merge) and split (the piece merge), with empty pieces (num_splits 8
    over one tile) and rows that see no key (len 1 under Sq 4 and 16) included."""
    lo, hi = _interval_t(DLENS, None, DB, sq, DCAP, window)
    for d, levels, splits in ((128, LEVELS, SPLITS), (64, LEVELS[:1], (0, 3))):
        for qval, kval in levels:
            score = wr.census_score(qval, kval, d)
            sinks, m = sr.census_sinks(hq, score)
            q, k, v, counts = wr.census_qkv((DB, hq, sq, d), (DB, hkv, DCAP, d), qval, kval, "stripe", dtype, DEV)
            for ns in splits:
                what = f"decode census {dr.name(dtype)} Hq={hq} Sq={sq} d={d} W={window} s={score:.2f} ns={ns}"
                base = _decode_form("contig", 0, q, k, v, DLENS, window, ns, _dev32(sinks))
                sr.check_census(base[0], lo, hi, counts, score, m, what, lse=base[1]).require()
                if d == 128 and qval:
                    for form, ps in (("paged", 64), ("contig_kv8", 0), ("paged_kv8", 128)):
                        got = _decode_form(form, ps, q, k, v, DLENS, window, ns, _dev32(sinks))
                        assert dr.same(got, base), f"{what} {form} page={ps}"
    assert dr.ws_counters_zero()


# ---- 2. dominant and negligible sinks ----------------------------------------------------

def _tiny(dtype):
    fi = torch.finfo(dtype)
    return fi.smallest_normal * fi.eps  # the smallest subnormal: one ulp of zero


@pytest.mark.parametrize("dtype", dr.DTYPES)
def test_dominant_and_negligible_sinks(dtype):
    """Every score -181.02 (Q = +4, K = -4, D = 128).  sinks = 0 lies 181 above
    them (261 in log2 units, past what 2^(sink2 - m_ref) alone can hold): O is
    zero to one ulp of zero and LSE = logaddexp(s + log n, 0), finite.  sinks =
    -400 lies 219 below: the result is the entry's without sinks."""
    d = 128
    score = wr.census_score(4.0, -4.0, d)
    gate = 2.0 ** -10 * abs(score) + 1e-5
    q, k, v, counts = wr.census_qkv((B, HQ, SQ, d), (B, HKV, CAP, d), 4.0, -4.0, "stripe", dtype, DEV)
    qd, kd, vd, dcounts = wr.census_qkv((DB, 6, 4, d), (DB, 2, DCAP, d), 4.0, -4.0, "stripe", dtype, DEV)
    runs = [(f"prefill W={w}", KV_LENS, Q_LENS, CAP, w, counts,
             lambda s, w=w: _prefill_form("contig", 0, q, k, v, KV_LENS, Q_LENS, w, s)) for w in (40, 0)]
    dlens = (5, 130, 1000)  # (no row without keys: its LSE is the sink, which the twin's census does not expect)
    runs += [(f"decode ns={ns}", dlens, None, DCAP, 100, dcounts,
              lambda s, ns=ns: _decode_form("contig", 0, qd, kd, vd, dlens, 100, ns, s)) for ns in (1, 3)]
    for what, kv_lens, q_lens, cap, w, cnt, run in runs:
        hq = 6 if q_lens is None else HQ
        o, lse = run(_dev32([0.0] * hq))
        b, sq = o.shape[0], o.shape[2]
        lo, hi = _interval_t(kv_lens, q_lens, b, sq, cap, w)
        n = (hi - lo).clamp(min=0).double().expand(b, hq, sq)
        want = torch.where(n > 0, torch.logaddexp(score + torch.log(n.clamp(min=1)), torch.zeros_like(n)),
                           torch.zeros_like(n))
        for bi, nb in enumerate(pr.n_rows(q_lens, b, sq)):
            omax = float(o[bi, :, :nb].float().abs().max())
            lerr = float((lse[bi, :, :nb].double().cpu() - want[bi, :, :nb]).abs().max())
            print(f"{what} {dr.name(dtype)} b={bi} dominant: max|O| {omax:.3e} lse err {lerr:.3e} gate {gate:.3e}")
            assert omax <= _tiny(dtype), (what, bi, omax)
            assert bool(torch.isfinite(lse[bi, :, :nb]).all()) and lerr <= gate, (what, bi, lerr)
        o, lse = run(_dev32([-400.0] * hq))
        for bi, nb in enumerate(pr.n_rows(q_lens, b, sq)):
            wr.check_census(o[bi, :, :nb], lo[bi, :, :nb], hi[bi, :, :nb], cnt, score,
                            f"{what} {dr.name(dtype)} b={bi} negligible", lse=lse[bi, :, :nb]).require()


# ---- 3. random inputs against the references ---------------------------------------------

RB, RHQ, RHKV, RSQ, RCAP = 2, 4, 2, 161, 320
RQ_LENS, RKV_LENS = (161, 130), (261, 230)   # behind a 100-key prefix: two query blocks


def _quant(x, scale):
    s = _dev32(scale)[None, :, None, None]
    x8 = (x / s).to(FP8)
    assert bool(torch.isfinite(x8.float()).all())
    return x8, x8.float() * s


@functools.lru_cache(maxsize=None)
def _inputs(b, hq, hkv, sq, cap, d, dtype, kv8):
    """(host fp16 bits, clean device (q, k, v) the references read, FP8 caches
    and scales or None).  kv8: the references see the dequantised cache."""
    q, k, v = dr.inputs(b, hq, hkv, sq, cap, d)
    tq = dr.dev(q).to(dtype)
    if not kv8:
        return (q, k, v), (tq, dr.dev(k).to(dtype), dr.dev(v).to(dtype)), None
    k8, kd = _quant(dr.dev(k).float(), K_SCALE)
    v8, vd = _quant(dr.dev(v).float(), V_SCALE)
    for x in (kd, vd):
        assert torch.equal(x.to(F16).float(), x) and torch.equal(x.to(BF16).float(), x)
    host = (q, dr.bits(kd.to(F16)), dr.bits(vd.to(F16)))
    return host, (tq, kd.to(dtype), vd.to(dtype)), (k8, v8, _dev32(K_SCALE), _dev32(V_SCALE))


@functools.lru_cache(maxsize=None)
def _refs(b, hq, hkv, sq, cap, d, dtype, kv8, kv_lens, q_lens, window, causal, seed):
    host, clean, _ = _inputs(b, hq, hkv, sq, cap, d, dtype, kv8)
    sinks = sr.draw_sinks(hq, seed)
    return sinks, sr.refs(host, clean, kv_lens, q_lens, window, dtype, sinks, causal)


@pytest.mark.parametrize("window,causal", [(0, True), (65, True), (0, False)])
@pytest.mark.parametrize("d", [128, 64])
@pytest.mark.parametrize("dtype", dr.DTYPES)
def test_prefill_random_inputs_against_the_references(dtype, d, window, causal):
    """Sinks drawn from N(0, 2) per head, the project's gates; paged equals
    contiguous and packed equals padded bit for bit; an FP8 cache with non-unit
    scales holds the gates on the dequantised cache (the sink takes neither
    scale: k_scale is 2^-6 and 2^-3 here)."""
    _, (q, k, v), _ = _inputs(RB, RHQ, RHKV, RSQ, RCAP, d, dtype, False)
    sinks, refs = _refs(RB, RHQ, RHKV, RSQ, RCAP, d, dtype, False, RKV_LENS, RQ_LENS, window, causal, 5)
    ts = _dev32(sinks)
    what = f"random {dr.name(dtype)} d={d} W={window} causal={causal}"
    base = _prefill_form("contig", 0, q, k, v, RKV_LENS, RQ_LENS, window, ts, causal=causal)
    sr.check(*base, refs, RQ_LENS, dtype, what)
    got = _prefill_form("paged", 128, q, k, v, RKV_LENS, RQ_LENS, window, ts, causal=causal)
    assert _same_rows(got, base, RQ_LENS), what
    # packed: the same rows, token-major
    cu = vr.cu_of(RQ_LENS)
    qp = vr.pack(q, RQ_LENS, total=cu[-1] + 7, fill=dr.NAN_BITS)
    po, pl = prefill_varlen(qp, _pad(k, RKV_LENS), _pad(v, RKV_LENS), _lens(cu), _lens(RKV_LENS), causal=causal,
                            return_lse=True, window=window, sinks=ts)
    packed = (vr.unpack(po, cu, RSQ), vr.unpack(pl, cu, RSQ, fill=NINF))
    assert _same_rows(packed, base, RQ_LENS), what + " packed"
    # an FP8 cache with non-unit scales
    _, (q8, k8, v8), sc = _inputs(RB, RHQ, RHKV, RSQ, RCAP, d, dtype, True)
    sinks8, refs8 = _refs(RB, RHQ, RHKV, RSQ, RCAP, d, dtype, True, RKV_LENS, RQ_LENS, window, causal, 6)
    base8 = _prefill_form("contig_kv8", 0, q8, k8, v8, RKV_LENS, RQ_LENS, window, _dev32(sinks8), sc, causal)
    sr.check(*base8, refs8, RQ_LENS, dtype, what + " fp8")
    got8 = _prefill_form("paged_kv8", 64, q8, k8, v8, RKV_LENS, RQ_LENS, window, _dev32(sinks8), sc, causal)
    assert _same_rows(got8, base8, RQ_LENS), what + " fp8 paged"
    kp, vp, table = _paginate(sc[0], sc[1], 64, RKV_LENS, seed=9)
    po, pl = prefill_varlen_paged(qp, kp, vp, table, _lens(cu), _lens(RKV_LENS), causal=causal, return_lse=True,
                                  window=window, sinks=_dev32(sinks8), k_scale=sc[2], v_scale=sc[3])
    packed = (vr.unpack(po, cu, RSQ), vr.unpack(pl, cu, RSQ, fill=NINF))
    assert _same_rows(packed, base8, RQ_LENS), what + " fp8 paged packed"


@pytest.mark.parametrize("dtype", dr.DTYPES)
def test_packed_prefill_over_a_contiguous_fp8_cache_against_the_references(dtype):
    """fa_prefill_varlen_sink_kv8_*, the one pair of sink entries nothing above
    calls (packed Q over a contiguous FP8 cache), at a small shape with real
    arguments: two sequences of 130 and 40 rows, the second behind a 30-key
    prefix, W = 80, non-unit scales; the gates on the dequantised cache."""
    b, hq, hkv, sq, cap, d, window = 2, 4, 2, 130, 192, 64, 80
    kv_lens, q_lens = (192, 70), (130, 40)
    _, (q, _, _), (k8, v8, ksc, vsc) = _inputs(b, hq, hkv, sq, cap, d, dtype, True)
    sinks, refs = _refs(b, hq, hkv, sq, cap, d, dtype, True, kv_lens, q_lens, window, True, 11)
    cu = vr.cu_of(q_lens)
    qp = vr.pack(q, q_lens, total=cu[-1] + 7, fill=dr.NAN_BITS)
    po, pl = prefill_varlen(qp, _pad(k8, kv_lens), _pad(v8, kv_lens), _lens(cu), _lens(kv_lens), return_lse=True,
                            window=window, sinks=_dev32(sinks), k_scale=ksc, v_scale=vsc)
    packed = (vr.unpack(po, cu, sq), vr.unpack(pl, cu, sq, fill=NINF))
    sr.check(*packed, refs, q_lens, dtype, f"packed fp8 contiguous {dr.name(dtype)} W={window}")


@pytest.mark.parametrize("dtype", dr.DTYPES)
def test_packed_prefill_over_a_paged_16_bit_pool_against_the_references(dtype):
    """fa_prefill_varlen_sink_paged_*, of which no Python function reached the
    bf16 entry (packed Q over 16-bit page pools), at the shape of the test above:
    the gates, and the contiguous packed call's result bit for bit."""
    b, hq, hkv, sq, cap, d, window = 2, 4, 2, 130, 192, 64, 80
    kv_lens, q_lens = (192, 70), (130, 40)
    _, (q, k, v), _ = _inputs(b, hq, hkv, sq, cap, d, dtype, False)
    sinks, refs = _refs(b, hq, hkv, sq, cap, d, dtype, False, kv_lens, q_lens, window, True, 12)
    cu = vr.cu_of(q_lens)
    qp = vr.pack(q, q_lens, total=cu[-1] + 7, fill=dr.NAN_BITS)
    kw = dict(return_lse=True, window=window, sinks=_dev32(sinks))
    kp, vp, table = _paginate(k, v, 64, kv_lens, seed=13)
    po, pl = prefill_varlen_paged(qp, kp, vp, table, _lens(cu), _lens(kv_lens), **kw)
    packed = (vr.unpack(po, cu, sq), vr.unpack(pl, cu, sq, fill=NINF))
    sr.check(*packed, refs, q_lens, dtype, f"packed paged {dr.name(dtype)} W={window}")
    co, cl = prefill_varlen(qp, _pad(k, kv_lens), _pad(v, kv_lens), _lens(cu), _lens(kv_lens), **kw)
    assert _same_rows(packed, (vr.unpack(co, cu, sq), vr.unpack(cl, cu, sq, fill=NINF)), q_lens)


@pytest.mark.parametrize("window,causal", [(0, True), (100, True), (0, False)])
@pytest.mark.parametrize("sq", [1, 4, 16])
@pytest.mark.parametrize("dtype", dr.DTYPES)
def test_decode_random_inputs_against_the_references(dtype, sq, window, causal):
    """Hq = 8 over Hkv = 2 (Sq 16: 64 rows, four heads in a workgroup), every
    num_splits, paged equal to contiguous bit for bit, and an FP8 cache with
    non-unit scales."""
    d, hq, hkv = 128, 8, 2
    _, (q, k, v), _ = _inputs(DB, hq, hkv, sq, DCAP, d, dtype, False)
    sinks, refs = _refs(DB, hq, hkv, sq, DCAP, d, dtype, False, DLENS, None, window, causal, 7)
    ts = _dev32(sinks)
    for ns in SPLITS:
        what = f"decode random {dr.name(dtype)} Sq={sq} W={window} causal={causal} ns={ns}"
        base = _decode_form("contig", 0, q, k, v, DLENS, window, ns, ts, causal=causal)
        sr.check(*base, refs, None, dtype, what)
        got = _decode_form("paged", 128, q, k, v, DLENS, window, ns, ts, causal=causal)
        assert dr.same(got, base), what
    _, (q8, k8, v8), sc = _inputs(DB, hq, hkv, sq, DCAP, d, dtype, True)
    sinks8, refs8 = _refs(DB, hq, hkv, sq, DCAP, d, dtype, True, DLENS, None, window, causal, 8)
    for form, ps, ns in (("contig_kv8", 0, 0), ("paged_kv8", 128, 3)):
        got = _decode_form(form, ps, q8, k8, v8, DLENS, window, ns, _dev32(sinks8), sc, causal)
        sr.check(*got, refs8, None, dtype, f"decode fp8 {form} {dr.name(dtype)} Sq={sq} W={window} causal={causal}")


# ---- the C entries through ctypes --------------------------------------------------------

def _c_entry(fam, paged, variant, extra, q, k, v, o, lse, b, hq, hkv, sq, table, kv_lens, second, causal, ns=1,
             ws=None, cap=None, rc_want=0):
    """One call of fa_<fam><variant>[_paged]_<dtype> through ctypes.  variant: "",
    "_win" or "_sink"; extra: what follows `causal` ((), (window,), (window,
    sinks tensor or None)).  second: q_lens / cu_seqlens_q.  k, v None: NULL
    caches (cap gives the capacity, or the pages per sequence)."""
    lib = fa_mi355x.load_library()
    fn = getattr(lib, fam + variant + ("_paged" if paged else "") + ("_bf16" if q.dtype is BF16 else "_f16"))
    d = q.shape[-1]
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    if paged:
        cache = (d, k.shape[0] if k is not None else 4, k.shape[2] if k is not None else 64, ptr(table),
                 table.shape[1] if cap is None else cap)
    else:
        cache = (k.shape[2] if cap is None else cap, d)
    ex = tuple(ptr(x) if isinstance(x, torch.Tensor) or x is None else x for x in extra)
    st = torch.cuda.current_stream().cuda_stream
    if fam == "fa_decode":
        rc = fn(ptr(q), ptr(k), ptr(v), ptr(o), ptr(lse), b, hq, hkv, sq, *cache, ptr(kv_lens), causal, *ex, ns,
                ptr(ws), 0 if ws is None else ws.numel(), st)
    else:
        rc = fn(ptr(q), ptr(k), ptr(v), ptr(o), ptr(lse), b, hq, hkv, sq, *cache, ptr(kv_lens), ptr(second),
                causal, *ex, st)
    assert rc == rc_want, (fam, paged, variant, causal, rc)


# ---- 4. rows without keys ------------------------------------------------------------------

SENT = 0x7bff  # fp16 65504 / a large bf16: what a row that must stay unwritten holds


def _sentinel(shape, dtype):
    t = torch.empty(shape, dtype=dtype, device=DEV)
    t.view(torch.int16).fill_(SENT)
    return t


def _check_keyless(o, lse, sinks, what):
    """o [Hq, rows, D], lse [Hq, rows] of rows that see no key: zeros, and the
    head's sink (exactly -inf where it is -inf)."""
    assert int(torch.count_nonzero(o)) == 0, what
    want = torch.as_tensor(sinks, dtype=torch.float64)[:, None].expand(lse.shape)
    got = lse.double().cpu()
    assert torch.equal(torch.isneginf(got), torch.isneginf(want)), what
    fin = torch.isfinite(want)
    err = float((got[fin] - want[fin]).abs().max())
    gate = 2.0 ** -10 * float(want[fin].abs().max()) + 1e-5
    print(f"{what}: lse err {err:.3e} gate {gate:.3e}")
    assert err <= gate, (what, err)


@pytest.mark.parametrize("paged", [False, True], ids=["contig", "paged"])
@pytest.mark.parametrize("dtype", dr.DTYPES)
def test_rows_without_keys(dtype, paged):
    """kv_lens[b] = 0 and kv_lens[b] < q_lens[b] (rows above the diagonal), in
    prefill, packed prefill and decode (split and not): O = 0 and LSE = sinks[h],
    -inf for the head without a sink; rows past q_lens keep the sentinel."""
    d, hq, hkv, sq, cap = 64, 4, 2, 130, 128
    sinks = [1.5, NINF, -3.0, 40.0]
    ts = _dev32(sinks)
    kv_lens, q_lens = (0, 50), (100, 80)
    _, (q, k, v), _ = _inputs(2, hq, hkv, sq, cap, d, dtype, False)
    table = None
    if paged:
        k, v, table = _paginate(k, v, 64, kv_lens, seed=3)
    else:
        k, v = _pad(k, kv_lens), _pad(v, kv_lens)
    o, lse = _sentinel(q.shape, dtype), torch.full((2, hq, sq), 7.0, dtype=torch.float32, device=DEV)
    _c_entry("fa_prefill", paged, "_sink", (0, ts), q, k, v, o, lse, 2, hq, hkv, sq, table, _lens(kv_lens),
             _lens(q_lens), 1)
    torch.cuda.synchronize()
    _check_keyless(o[0, :, :100], lse[0, :, :100], sinks, "prefill len 0")
    _check_keyless(o[1, :, :30], lse[1, :, :30], sinks, "prefill above the diagonal")
    assert bool(torch.isfinite(lse[1, :, 30:80]).all()) and int(torch.count_nonzero(o[1, :, 30:80])) > 0
    for bi, n in enumerate(q_lens):
        assert bool((o[bi, :, n:].view(torch.int16) == SENT).all()) and bool((lse[bi, :, n:] == 7.0).all()), bi
    # packed: the same rows
    cu = vr.cu_of(q_lens)
    qp = vr.pack(q, q_lens, total=cu[-1] + 3, fill=dr.NAN_BITS)
    po, pl = _sentinel(qp.shape, dtype), torch.full((hq, qp.shape[0]), 7.0, dtype=torch.float32, device=DEV)
    _c_entry("fa_prefill_varlen", paged, "_sink", (0, ts), qp, k, v, po, pl, 2, hq, hkv, qp.shape[0], table,
             _lens(kv_lens), _lens(cu), 1)
    torch.cuda.synchronize()
    for bi, n in enumerate(q_lens):
        rows = slice(cu[bi], cu[bi] + n)
        assert torch.equal(po[rows].transpose(0, 1), o[bi, :, :n]) and torch.equal(pl[:, rows], lse[bi, :, :n]), bi
    assert bool((po[cu[-1]:].view(torch.int16) == SENT).all()) and bool((pl[:, cu[-1]:] == 7.0).all())
    # decode: Sq 4 over lengths 0 and 2
    dq = q[:, :, :4].contiguous()
    dlens = (0, 2)
    ws = torch.zeros(1 << 21, dtype=torch.uint8, device=DEV)
    if paged:
        dk, dv, dtable = _paginate(_inputs(2, hq, hkv, sq, cap, d, dtype, False)[1][1],
                                   _inputs(2, hq, hkv, sq, cap, d, dtype, False)[1][2], 64, dlens, seed=4)
    else:
        dk, dv, dtable = _pad(k, dlens), _pad(v, dlens), None
    for ns in (1, 3):
        o, lse = _sentinel(dq.shape, dtype), torch.full((2, hq, 4), 7.0, dtype=torch.float32, device=DEV)
        _c_entry("fa_decode", paged, "_sink", (0, ts), dq, dk, dv, o, lse, 2, hq, hkv, 4, dtable, _lens(dlens),
                 None, 1, ns, ws)
        torch.cuda.synchronize()
        _check_keyless(o[0], lse[0], sinks, f"decode len 0 ns={ns}")
        _check_keyless(o[1, :, :2], lse[1, :, :2], sinks, f"decode above the diagonal ns={ns}")
        assert bool(torch.isfinite(lse[1, :, 2:]).all())
    assert int(torch.count_nonzero(ws[:65536])) == 0


@pytest.mark.parametrize("paged", [False, True], ids=["contig", "paged"])
@pytest.mark.parametrize("fam", sr.FAMILIES)
def test_zero_capacity_through_the_c_entry(fam, paged):
    """kv_capacity = 0 (paged: no pages per sequence), NULL caches: the early
    fill writes O = 0 and LSE = sinks[h] (bit for bit: it copies the value), -inf
    for the head without a sink, and -inf everywhere with sinks = NULL as the
    twin does."""
    d, b, hq, hkv = 128, 2, 4, 2
    sinks = [1.5, NINF, -3.0, 40.0]
    ts = _dev32(sinks)
    sq = 3 if fam == "fa_decode" else 70
    table = torch.zeros((b, 1), dtype=torch.int32, device=DEV) if paged else None
    if fam == "fa_prefill_varlen":
        q = dr.rand((sq, hq, d), F16, 1)
        lse_shape, head_axis = (hq, sq), 0
        second = _lens([0, 30, sq])
    else:
        q = dr.rand((b, hq, sq, d), F16, 1)
        lse_shape, head_axis = (b, hq, sq), 1
        second = None
    for s in (ts, None):
        o = dr.nan_fill(torch.empty_like(q))
        lse = torch.full(lse_shape, float("nan"), dtype=torch.float32, device=DEV)
        _c_entry(fam, paged, "_sink", (0, s), q, None, None, o, lse, b, hq, hkv, sq, table, None, second, 1, cap=0)
        torch.cuda.synchronize()
        assert int(torch.count_nonzero(o)) == 0
        want = torch.tensor(sinks if s is not None else [NINF] * hq, dtype=torch.float32, device=DEV)
        shape = [1] * len(lse_shape)
        shape[head_axis] = hq
        assert torch.equal(lse, want.view(shape).expand(lse_shape)), (fam, paged, s is None)


# ---- 5. bit identity -----------------------------------------------------------------------

@pytest.mark.parametrize("paged", [False, True], ids=["contig", "paged"])
@pytest.mark.parametrize("fam", sr.FAMILIES)
@pytest.mark.parametrize("dtype", dr.DTYPES)
def test_sink_entries_without_sinks_equal_their_twins(dtype, fam, paged):
    """A `_sink` entry with sinks = NULL, and with every sink -inf, computes what
    its `_win` twin computes, O and LSE bit for bit, at window 0 and 40 (decode:
    unsplit and split).  And the Python functions with sinks=None still take the
    plain entry (window 0) and the `_win` entry."""
    d, hq, hkv = 128, 8, 2
    if fam == "fa_decode":
        b, sq, cap, kv_lens, n = DB, 4, DCAP, DLENS, None
    else:
        b, sq, cap, kv_lens, n = RB, RSQ, RCAP, RKV_LENS, RQ_LENS
    _, (q, k, v), _ = _inputs(b, hq, hkv, sq, cap, d, dtype, False)
    table = None
    if paged:
        k, v, table = _paginate(k, v, 64, kv_lens, seed=4)
    else:
        k, v = _pad(k, kv_lens), _pad(v, kv_lens)
    tl = _lens(kv_lens)
    if fam == "fa_prefill_varlen":
        cu = vr.cu_of(n)
        q = vr.pack(q, n, total=cu[-1] + 5, fill=dr.NAN_BITS)
        second, rows, lse_shape = _lens(cu), q.shape[0], (hq, q.shape[0])
        own = torch.from_numpy(vr.owned_rows(cu, rows)).to(DEV)
    else:
        second, rows, lse_shape = _lens(n), sq, (b, hq, sq)
    ws = torch.zeros(1 << 22, dtype=torch.uint8, device=DEV) if fam == "fa_decode" else None
    ninf = _dev32([NINF] * hq)

    def run(variant, extra, ns):
        o = dr.nan_fill(torch.empty_like(q))
        lse = torch.full(lse_shape, float("nan"), dtype=torch.float32, device=DEV)
        _c_entry(fam, paged, variant, extra, q, k, v, o, lse, b, hq, hkv, rows, table, tl, second, 1, ns, ws)
        torch.cuda.synchronize()
        return o, lse

    def same(a, c):
        if fam == "fa_prefill_varlen":
            return torch.equal(a[0][own], c[0][own]) and torch.equal(a[1][:, own], c[1][:, own])
        if fam == "fa_prefill":
            return _same_rows(a, c, n)
        return dr.same(a, c)

    for w in (0, 40):
        for ns in ((1, 3) if fam == "fa_decode" else (1,)):
            twin = run("_win", (w,), ns)
            assert same(run("_sink", (w, None), ns), twin), (w, ns, "NULL")
            assert same(run("_sink", (w, ninf), ns), twin), (w, ns, "-inf")
            # the Python function without sinks: the plain entry at W = 0, the `_win` entry at 40
            kw = dict(return_lse=True, window=w, sinks=None)
            if fam == "fa_decode":
                py = (decode_paged(q, k, v, table, tl, num_splits=ns, **kw) if paged
                      else decode(q, k, v, tl, num_splits=ns, **kw))
            elif fam == "fa_prefill":
                py = (prefill_paged(q, k, v, table, tl, second, **kw) if paged
                      else prefill(q, k, v, tl, second, **kw))
            else:
                py = (prefill_varlen_paged(q, k, v, table, second, tl, **kw) if paged
                      else prefill_varlen(q, k, v, second, tl, **kw))
            torch.cuda.synchronize()
            assert same(py, run("" if w == 0 else "_win", () if w == 0 else (w,), ns)), (w, ns, "python")


def test_sinks_on_another_device_or_the_host_are_refused():
    q, k = dr.rand((1, 4, 2, 64), F16, 1), dr.rand((1, 2, 64, 64), F16, 2)
    with pytest.raises(fa_mi355x.FlashAttentionError, match="sinks must be a tensor on cuda:0") as e:
        decode(q, k, k, sinks=torch.zeros(4))
    assert e.value.status == fa_mi355x.FA_ERR_NULL_POINTER
    with pytest.raises(fa_mi355x.FlashAttentionError, match=r"sinks must be a contiguous float32 \[Hq = 4\]"):
        prefill(q, k, k, sinks=torch.zeros(2, device=DEV))


# ---- 6. graphs ------------------------------------------------------------------------------

def _capture(fn):
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        fn()  # warm-up outside the capture
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            res = fn()
    torch.cuda.current_stream().wait_stream(stream)
    return graph, res


def test_captured_graphs_follow_rewritten_sinks_and_lengths():
    """One captured graph each of prefill and of (split) decode, replayed after
    sinks and kv_lens were rewritten in place: both are read on the device."""
    d, hq, hkv, w = 128, 8, 2, 65
    _, (q, k, v), _ = _inputs(RB, hq, hkv, RSQ, RCAP, d, F16, False)
    _, (qd, kd, vd), _ = _inputs(DB, hq, hkv, 4, DCAP, d, F16, False)
    sinks = [sr.draw_sinks(hq, 11), sr.draw_sinks(hq, 12) + 3.0]
    ts, tl, ql, dl = _dev32(sinks[0]), _lens(RKV_LENS), _lens(RQ_LENS), _lens(DLENS)
    out, dout = torch.empty_like(q), torch.empty_like(qd)
    gp, rp = _capture(lambda: prefill(q, k, v, tl, ql, out=out, return_lse=True, window=w, sinks=ts))
    gd, rd = _capture(lambda: decode(qd, kd, vd, dl, out=dout, return_lse=True, num_splits=3, window=w, sinks=ts))
    cases = ((sinks[0], RKV_LENS, RQ_LENS, DLENS), (sinks[1], (200, 77), (120, 40), (700, 3, 64)))
    for s, kv_lens, q_lens, dlens in cases:
        ts.copy_(_dev32(s))
        tl.copy_(_lens(kv_lens))
        ql.copy_(_lens(q_lens))
        dl.copy_(_lens(dlens))
        gp.replay()
        gd.replay()
        torch.cuda.synchronize()
        want = prefill(q, k, v, _lens(kv_lens), _lens(q_lens), return_lse=True, window=w, sinks=_dev32(s))
        assert _same_rows(rp, want, q_lens), kv_lens
        host, clean, _ = _inputs(RB, hq, hkv, RSQ, RCAP, d, F16, False)
        sr.check(*rp, sr.refs(host, clean, kv_lens, q_lens, w, F16, s), q_lens, F16, f"graph prefill {kv_lens}")
        want = decode(qd, kd, vd, _lens(dlens), return_lse=True, num_splits=3, window=w, sinks=_dev32(s))
        assert dr.same(rd, want), dlens
        host, clean, _ = _inputs(DB, hq, hkv, 4, DCAP, d, F16, False)
        sr.check(*rd, sr.refs(host, clean, dlens, None, w, F16, s), None, F16, f"graph decode {dlens}")


# ---- 7. the loop ----------------------------------------------------------------------------

@pytest.mark.parametrize("window", [128, 0])
@pytest.mark.parametrize("paged", [False, True], ids=["contig", "paged"])
@pytest.mark.parametrize("dtype", dr.DTYPES)
def test_serving_loop_prefill_append_decode_with_sinks(dtype, paged, window):
    """The gpt-oss layer pair (a 128-key window layer and a full-attention layer,
    both with sinks) at Hq = 8, Hkv = 1, D = 64: prefill of a 200-token chunk
    behind 100 cached keys, one token appended, decode of it -- each step against
    the float64 contract on the cache as it then stands."""
    d, hq, hkv, b, cap, pre, n = 64, 8, 1, 2, 384, 100, 200
    _, (q, k, v), _ = _inputs(b, hq, hkv, n, cap, d, dtype, False)
    q1 = _inputs(b, hq, hkv, 1, cap, d, dtype, False)[1][0]
    sinks = sr.draw_sinks(hq, 21)
    ts = _dev32(sinks)
    lens0, lens1 = (pre + n, pre + n - 9), (pre + n + 1, pre + n - 8)
    ql = (n, n - 9)
    if paged:
        kc, vc, table = _paginate(k, v, 128, (cap, cap), seed=5)
        pf = lambda *a, **kw: prefill_paged(q, kc, vc, table, *a, **kw)          # noqa: E731
        dc = lambda *a, **kw: decode_paged(q1, kc, vc, table, *a, **kw)          # noqa: E731
        ap = lambda kn, vn, tl: fa_mi355x.flash_attention_cache_append_paged(kn, vn, kc, vc, table, tl)  # noqa: E731
        full = lambda: (dr.gather(kc, table), dr.gather(vc, table))              # noqa: E731
    else:
        kc, vc = k.clone(), v.clone()
        pf = lambda *a, **kw: prefill(q, kc, vc, *a, **kw)                       # noqa: E731
        dc = lambda *a, **kw: decode(q1, kc, vc, *a, **kw)                       # noqa: E731
        ap = lambda kn, vn, tl: fa_mi355x.flash_attention_cache_append(kn, vn, kc, vc, tl)  # noqa: E731
        full = lambda: (kc, vc)                                                  # noqa: E731

    def contract(qq, kv_lens, q_lens):
        kf, vf = full()
        o, lse, _, smax = sr.contract_f64(qq.double().cpu().numpy(), kf.double().cpu().numpy(),
                                          vf.double().cpu().numpy(), kv_lens, q_lens, window, sinks,
                                          with_smax=True)
        return np.nan_to_num(o), np.nan_to_num(lse, neginf=NINF), smax

    got = pf(_lens(lens0), _lens(ql), return_lse=True, window=window, sinks=ts)
    sr.check(*got, contract(q, lens0, ql), ql, dtype, f"loop prefill W={window}")
    gen = torch.Generator(device=DEV).manual_seed(9)
    kn = (torch.rand((b, hkv, 1, d), generator=gen, device=DEV) - 0.5).to(dtype)
    vn = (torch.rand((b, hkv, 1, d), generator=gen, device=DEV) - 0.5).to(dtype)
    ap(kn, vn, _lens(lens1))
    kf, _ = full()
    for bi in range(b):
        assert torch.equal(kf[bi, :, lens1[bi] - 1], kn[bi, :, 0])
    for ns in (0, 2):
        got = dc(_lens(lens1), return_lse=True, num_splits=ns, window=window, sinks=ts)
        sr.check(*got, contract(q1, lens1, None), None, dtype, f"loop decode W={window} ns={ns}")
