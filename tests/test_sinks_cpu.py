"""CPU tests of attention sinks (no GPU): the float64 restatement of the
contract with sinks against the two references the GPU tests use, at half of
each of their gates; the census expectation with sinks and the bound that makes
a miscounted sink visible; the 24 fa_*_sink_* entries' symbols, argument lists
and statuses (all returned before any launch, so fake pointers suffice); the
Python wrappers' rejections; the `.sinks` torch ops beside the unchanged
schemas; and the compile-time resource usage of the twelve new units.
"""
import ctypes
import math
import os
import re
import types

import numpy as np
import pytest
import torch

import capi_checks as cc
import decode_refs as dr
import fa_mi355x
import prefill_refs as pr
import sink_refs as sr
import window_refs as wr

INT_MAX = cc.INT_MAX
P = ctypes.c_void_p(0x1000)
err = fa_mi355x.FlashAttentionError
NINF = float("-inf")

ENTRIES = [(fam, paged, kv8, bf16) for fam in sr.FAMILIES for paged in (False, True) for kv8 in (False, True)
           for bf16 in (False, True)]


def _symbol(entry, variant="_sink"):
    fam, paged, kv8, bf16 = entry
    return sr.symbol(fam, ("_paged" if paged else "") + ("_kv8" if kv8 else ""), bf16, variant)


SYMBOLS = [_symbol(e) for e in ENTRIES]


def test_symbols_exported_and_declared():
    assert len(set(SYMBOLS)) == 24
    cc.assert_exported(SYMBOLS)
    header = open(os.path.join(cc.ROOT, "include", "fa_mi355x.h")).read()
    for e in ENTRIES:
        # the `_win` twin's argument list with `const float* sinks` directly after `int window`
        a, b = (" ".join(re.search(r"\b%s\s*\((.*?)\)" % _symbol(e, v), header, re.S).group(1).split())
                for v in ("_win", "_sink"))
        assert b == a.replace("int window,", "int window, const float* sinks,"), _symbol(e)
    lib = fa_mi355x.load_library()
    for e in ENTRIES:
        a, b = (getattr(lib, _symbol(e, v)).argtypes for v in ("_win", "_sink"))
        at = [i for i in range(len(b)) if b[:i] + b[i + 1:] == a and b[i] is ctypes.c_void_p]
        assert at and b[at[0] - 1] is ctypes.c_int, _symbol(e)


# ---- the contract, restated, against the references ------------------------------------

def _f64_bits(a):
    return a.view(np.float16).astype(np.float64)


SINK_SETS = {
    "drawn": lambda hq: sr.draw_sinks(hq),
    "one_head_without": lambda hq: torch.cat([sr.draw_sinks(hq)[:1], torch.tensor([NINF]), sr.draw_sinks(hq)[2:]]),
    "dominant": lambda hq: torch.full((hq,), 30.0),
}


@pytest.mark.parametrize("which", sorted(SINK_SETS))
@pytest.mark.parametrize("window,causal", [(0, True), (5, True), (64, True), (0, False)])
def test_restatement_against_the_references(window, causal, which):
    """contract_f64 with the sink column (its own arithmetic) against the
    CPU-oracle rows carried over by the two identities and fp32 torch with an
    explicit extra column, each at HALF the gate the GPU tests hold the kernels
    to, and the float64 LSE by logaddexp; ragged q_lens, a negative off_b, an
    element whose leading rows see no key."""
    b, hq, hkv, sq, cap, d = 3, 4, 2, 40, 192, 64
    kv_lens, q_lens = (150, 20, 192), (40, 33, 7)
    sinks = SINK_SETS[which](hq)
    q, k, v = dr.inputs(b, hq, hkv, sq, cap, d)
    o, lse, written, smax = sr.contract_f64(_f64_bits(q), _f64_bits(k), _f64_bits(v), kv_lens, q_lens, window,
                                            sinks, causal, with_smax=True)
    tq, tk, tv = (torch.from_numpy(np.array(a).view(np.int16)).view(torch.float16) for a in (q, k, v))
    ro, lref, smax2 = sr.refs((q, k, v), (tq, tk, tv), kv_lens, q_lens, window, torch.float16, sinks, causal)
    to, tl = sr.ref_torch(tq, tk, tv, kv_lens, window, q_lens, sinks, causal)
    assert abs(smax - smax2) <= 1e-6 * max(1.0, smax)
    w3 = np.broadcast_to(written[:, None, :], lse.shape)
    e_or = float(np.abs(ro[w3] - o[w3]).max())
    e_to = float(np.abs(to.double().numpy()[w3] - o[w3]).max())
    live = w3 & np.isfinite(lse)
    e_l = float(np.abs(lref[live] - lse[live]).max())
    e_tl = float(np.abs(tl.double().numpy()[live] - lse[live]).max())
    print(f"W={window} causal={causal} {which}: oracle {e_or:.2e} torch {e_to:.2e} lse {e_l:.2e} torch lse {e_tl:.2e}")
    assert e_or <= dr.GATE_F16 / 2 and e_to <= dr.GATE_BF16 / 2 and e_to <= 1e-5
    assert e_l <= 1e-10 and e_tl <= sr.lse_gate(smax) / 2
    assert np.array_equal(np.isneginf(lref) & w3, np.isneginf(lse) & w3)
    # rows that see no key: zeros and the head's sink (element 1 when causal: 20 keys, 33 rows)
    lo, hi = wr.interval(kv_lens, q_lens, b, sq, cap, window)
    if causal:
        unseen = (hi == lo) & written
        assert unseen[1, :13].all() and unseen.sum() == 13
        for h in range(hq):
            assert (lse[1, h, :13] == float(sinks[h])).all() and not o[1, h, :13].any()
    # sinks=None and all -inf: the contract without sinks, bit for bit in float64
    if causal:
        o0, l0, w0 = wr.contract_f64(_f64_bits(q), _f64_bits(k), _f64_bits(v), kv_lens, q_lens, window)
    else:
        o0, l0, w0 = pr.contract_f64(_f64_bits(q), _f64_bits(k), _f64_bits(v), kv_lens, q_lens, False)
    for none in (None, [NINF] * hq):
        o1, l1, w1 = sr.contract_f64(_f64_bits(q), _f64_bits(k), _f64_bits(v), kv_lens, q_lens, window, none, causal)
        assert np.array_equal(w0, w1)
        assert np.abs(o1[w3] - o0[w3]).max() <= 1e-14 and np.array_equal(np.isneginf(l0), np.isneginf(l1))
        fin = w3 & np.isfinite(l0)
        assert np.abs(l1[fin] - l0[fin]).max() <= 1e-12


def test_identities_at_the_extremes():
    """transform(): a sink far above every score gives O -> 0 and LSE -> sink, one
    far below changes nothing, -inf beside a row without keys stays 0 / -inf."""
    o0 = np.ones((1, 3, 2, 4))
    l0 = np.array([[[-181.0, NINF], [-181.0, NINF], [-181.0, NINF]]])
    o, lse = sr.transform(o0, l0, [0.0, -400.0, NINF])
    assert o[0, 0].max() < 1e-70 and abs(lse[0, 0, 0]) < 1e-70 and lse[0, 0, 1] == 0.0
    assert np.array_equal(o[0, 1, 0], o0[0, 1, 0]) and lse[0, 1, 0] == -181.0 and lse[0, 1, 1] == -400.0
    assert not o[0, 1, 1].any() and not o[0, 2, 1].any()
    assert np.array_equal(o[0, 2, 0], o0[0, 2, 0]) and lse[0, 2, 0] == -181.0 and lse[0, 2, 1] == NINF


# ---- census with sinks ------------------------------------------------------------------

# the GPU tests' census shapes (tests/test_sinks_gpu.py)
PRE = dict(b=pr.KS_B, hq=4, hkv=2, sq=pr.KS_SQ, cap=pr.KS_CAP, kv_lens=pr.KS_KV_LENS, q_lens=pr.KS_Q_LENS,
           windows=(0, 40, 128, 130))
DEC = dict(b=3, cap=1024, kv_lens=(1, 130, 1000), windows=(0, 5, 64, 100),
           geoms=((6, 2, 1), (6, 2, 4), (6, 2, 16), (16, 2, 16)))
BOUND = 250  # n + m_max where a window or a length cuts: a miscounted sink moves O by >= 1 / 251 = 4.08 * 2^-10


def test_census_bound_of_the_gpu_shapes():
    """n + m_max <= 250 on every row of every windowed case, and on the rows of
    the short elements without a window, so a sink dropped, doubled or taken
    from a neighbouring head moves a denominator by >= 1 / (n + m_max + 1) >= 4
    fp16 gates (2^-10).  (bf16's gate is 2^-7: there the W <= 5 and short-length
    rows carry the signal, n + m_max + 1 <= 32.)"""
    m_max = int(sr.census_sinks(PRE["hq"], 0.0)[1].max())
    assert m_max == 7
    for w in PRE["windows"]:
        lo, hi = wr.interval(PRE["kv_lens"], PRE["q_lens"], PRE["b"], PRE["sq"], PRE["cap"], w)
        n = (hi - lo)[hi >= 0]
        if w:
            assert n.max() + m_max <= BOUND and n.max() == w, w
            assert sr.census_signal(lo, hi, m_max) >= 4 * 2.0 ** -10
        else:
            assert (n + m_max <= BOUND).sum() >= 40  # the first rows behind the 200-key prefix
    for hq, hkv, sq in DEC["geoms"]:
        m_max = int(sr.census_sinks(hq, 0.0)[1].max())
        assert m_max == 2 * hq - 1 <= 31
        for w in DEC["windows"]:
            lo, hi = wr.interval(DEC["kv_lens"], None, DEC["b"], sq, DEC["cap"], w)
            n = hi - lo
            if w:
                assert n.max() + m_max <= BOUND, (hq, sq, w)
            else:
                assert n[:2].max() + m_max <= BOUND and n[2].min() > BOUND  # lengths 1 and 130 carry it
        lo, hi = wr.interval(DEC["kv_lens"], None, DEC["b"], sq, DEC["cap"], 5)
        assert (hi - lo).max() + m_max + 1 <= 37


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("qval,kval,d", [(0.0, 0.0, 64), (4.0, -4.0, 128)])
def test_census_expectation_with_sinks_holds_its_gate(dtype, qval, kval, d):
    """The closed form (n + m_h in the denominator, LSE = s + log(n + m_h))
    against the float64 restatement on the census inputs, at both score levels,
    so a miss on the GPU is the kernel's; and the checker sees a sink that is
    dropped, counted twice or taken from the neighbouring head."""
    b, hq, hkv, sq, cap, w = 1, 4, 2, 70, 256, 40
    kv_lens, q_lens = (230,), (70,)
    q, k, v, counts = wr.census_qkv((b, hq, sq, d), (b, hkv, cap, d), qval, kval, "stripe", dtype)
    score = wr.census_score(qval, kval, d)
    sinks, m = sr.census_sinks(hq, score)
    assert d != 128 or abs(score + 181.0193) < 1e-3
    lo, hi = wr.interval(kv_lens, q_lens, b, sq, cap, w)
    lo, hi = torch.from_numpy(lo)[:, None], torch.from_numpy(hi)[:, None]

    def run(sk):
        o, lse, _ = sr.contract_f64(q.double().numpy(), k.double().numpy(), v.double().numpy(), kv_lens, q_lens,
                                    w, sk)
        return torch.from_numpy(o).to(dtype).double(), torch.from_numpy(lse)  # the final rounding the gate allows

    o, lse = run(sinks)
    sr.check_census(o, lo, hi, counts, score, m, f"restatement {dtype}", lse=lse, dtype=dtype).require()
    assert abs(float(lse[0, 2, 0]) - (score + math.log(w + 5))) < 1e-4  # (float32 sinks)
    twice = torch.log(2 * m.double()).float() + score
    for name, bad in (("dropped", torch.full((hq,), NINF)), ("twice", twice), ("neighbour", sinks.roll(1))):
        res = sr.check_census(run(bad)[0], lo, hi, counts, score, m, name, dtype=dtype)
        assert not res.ok, name
    # without keys: O = 0 and LSE = the sink
    o, lse = sr.census_expected(counts, torch.zeros(hq, 1).long(), torch.zeros(hq, 1).long(), score, m[:, None])
    assert not o.any() and torch.allclose(lse[:, 0], sinks.double(), atol=1e-4)


# ---- the C entries' argument statuses ------------------------------------------------

def _call(entry, q, k, v, o, b, hq, hkv, sq, cap, d, lens=None, ql=None, cu=P, causal=1, window=5, sinks=P, ns=0,
          ws=None, wsb=0, table=P, npages=100, psz=128, mpp=None):
    fam, paged, kv8, _ = entry
    fn = getattr(fa_mi355x.load_library(), _symbol(entry))
    tail = (None, None) if kv8 else ()
    if paged:
        pages = cap // psz if mpp is None and psz > 0 else (mpp or 0)
        cache = (d, npages, psz, table, pages)
    else:
        cache = (cap, d)
    if fam == "fa_decode":
        return fn(q, k, v, o, None, b, hq, hkv, sq, *cache, lens, causal, window, sinks, ns, ws, wsb, None, *tail)
    second = cu if fam == "fa_prefill_varlen" else ql
    return fn(q, k, v, o, None, b, hq, hkv, sq, *cache, lens, second, causal, window, sinks, None, *tail)


@pytest.mark.parametrize("with_sinks", [True, False], ids=["sinks", "null"])
@pytest.mark.parametrize("entry", ENTRIES, ids=SYMBOLS)
def test_sink_argument_statuses(entry, with_sinks):
    """The `_win` twin's table (tests/test_window_cpu.py) replayed with `sinks`
    inserted, a pointer and NULL alike: sinks adds no status and moves none."""
    fa = fa_mi355x
    fam, paged, _, _ = entry
    call = lambda *a, **kw: _call(entry, *a, sinks=P if with_sinks else None, **kw)  # noqa: E731
    sq = 4 if fam == "fa_decode" else 300
    b = 3
    good = (b, 8, 2, sq, 1024, 128)
    for w in (0, 1, 64, 4096, INT_MAX):
        assert call(None, P, P, P, *good, window=w) == fa.FA_ERR_NULL_POINTER, w
    assert call(None, P, P, P, *good, window=0, causal=0) == fa.FA_ERR_NULL_POINTER
    for w in (-1, -INT_MAX - 1):
        assert call(P, P, P, P, *good, window=w) == fa.FA_ERR_BAD_SHAPE
        assert call(P, P, P, P, b, 8, 2, sq, 1024, 96, window=w) == fa.FA_ERR_BAD_SHAPE
        assert call(None, None, None, None, 0, 8, 2, sq, 1024, 128, window=w, table=None, cu=None) == \
            fa.FA_ERR_BAD_SHAPE
    assert call(P, P, P, P, *good, window=1, causal=0) == fa.FA_ERR_BAD_SHAPE
    assert call(P, P, P, P, b, 8, 2, sq, 1024, 96, window=1, causal=0) == fa.FA_ERR_UNSUPPORTED_HEAD_DIM
    assert call(None, None, None, None, 0, 8, 2, sq, 1024, 128, window=1, causal=0, table=None, cu=None) == \
        fa.FA_ERR_BAD_SHAPE
    assert call(None, None, None, None, 0, 8, 2, sq, 1024, 128, window=0, causal=0, table=None, cu=None) == \
        fa.FA_OK
    for bad in range(4):
        ptrs = [None if i == bad else P for i in range(4)]
        assert call(*ptrs, *good) == fa.FA_ERR_NULL_POINTER
    for d in (0, 32, 96, 256):
        assert call(P, P, P, P, b, 8, 2, sq, 1024, d) == fa.FA_ERR_UNSUPPORTED_HEAD_DIM
    for hq, hkv in ((8, 3), (7, 2), (4, 8)):
        assert call(P, P, P, P, b, hq, hkv, sq, 1024, 128) == fa.FA_ERR_BAD_SHAPE
    for x in ((-1, 8, 2), (b, -8, 2), (b, 8, -2)):
        assert call(P, P, P, P, *x, sq, 1024, 128) == fa.FA_ERR_BAD_SHAPE
    bad_sq = {"fa_decode": (0, 17, -1), "fa_prefill": (0, -1), "fa_prefill_varlen": (-1,)}[fam]
    for s in bad_sq:
        assert call(P, P, P, P, b, 8, 2, s, 1024, 128) == fa.FA_ERR_BAD_SHAPE, s
    if fam == "fa_prefill_varlen":
        assert call(P, P, P, P, *good, cu=None) == fa.FA_ERR_NULL_POINTER
        assert call(None, None, None, None, b, 8, 2, 0, 1024, 128, table=None, cu=None) == fa.FA_OK
        assert call(P, P, P, P, 1, 64, 64, 1 << 25, 1024, 128) == fa.FA_ERR_BAD_SHAPE
    if fam == "fa_prefill":
        assert call(P, P, P, P, 1, 8, 2, 1 << 23, 1024, 128) == fa.FA_ERR_BAD_SHAPE
    if paged:
        assert call(P, P, P, P, *good, table=None) == fa.FA_ERR_NULL_POINTER
        for psz in (0, 32, 96, -64, 1, 63, 65):
            assert call(P, P, P, P, *good, psz=psz, mpp=8) == fa.FA_ERR_BAD_SHAPE, psz
        for npages in (0, -1):
            assert call(P, P, P, P, *good, npages=npages) == fa.FA_ERR_BAD_SHAPE
        assert call(P, P, P, P, *good, mpp=-1) == fa.FA_ERR_BAD_SHAPE
        assert call(P, P, P, P, b, 8, 2, sq, 0, 128, psz=64, mpp=2147483520 // 64 + 1) == fa.FA_ERR_BAD_SHAPE
        assert call(P, P, P, P, b, 8, 2, sq, 0, 128, npages=1, psz=1 << 23, mpp=1) == fa.FA_ERR_BAD_SHAPE
        assert call(None, None, None, None, 0, 8, 2, sq, 1024, 128, table=None, psz=96, mpp=8, cu=None) == \
            fa.FA_ERR_BAD_SHAPE
    else:
        assert call(P, P, P, P, b, 8, 2, sq, -5, 128) == fa.FA_ERR_BAD_SHAPE
        assert call(P, P, P, P, b, 8, 2, sq, 8388608, 128) == fa.FA_ERR_BAD_SHAPE
        assert call(None, P, P, P, b, 8, 2, sq, 8388607, 128) == fa.FA_ERR_NULL_POINTER
    # empty problems; rows but no keys: only o is needed (and missing here)
    assert call(None, None, None, None, 0, 8, 2, sq, 1024, 128, table=None, cu=None) == fa.FA_OK
    assert call(None, None, None, None, b, 0, 0, sq, 1024, 128, table=None, cu=None) == fa.FA_OK
    assert call(None, None, None, None, b, 8, 2, sq, 0, 128, table=None, mpp=0, cu=None) == \
        fa.FA_ERR_NULL_POINTER


def _decode_shim(paged, kv8, window, sinks):
    """The loaded library with fa_decode[_paged]_f16 / _bf16 bound to the sink
    entries at a fixed window and sinks pointer, for capi_checks' decode tables."""
    lib = fa_mi355x.load_library()
    shim = types.SimpleNamespace(fa_decode_ws_bytes=lib.fa_decode_ws_bytes,
                                 fa_decode_num_splits=lib.fa_decode_num_splits)
    at = 15 if paged else 12  # the arguments up to and including causal

    def bind(fn):
        tail = (None, None) if kv8 else ()
        return lambda *a: fn(*a[:at + 1], window, sinks, *a[at + 1:], *tail)

    for ty in ("_f16", "_bf16"):
        name = "fa_decode" + ("_paged" if paged else "") + ty
        setattr(shim, name, bind(getattr(lib, sr.symbol("fa_decode", ("_paged" if paged else "")
                                                        + ("_kv8" if kv8 else ""), ty == "_bf16"))))
    return shim


@pytest.mark.parametrize("kv8", [False, True], ids=["16bit", "kv8"])
@pytest.mark.parametrize("paged", [False, True], ids=["contig", "paged"])
def test_decode_twins_tables_with_sinks(paged, kv8):
    """capi_checks' whole decode tables (workspace statuses included) hold for
    the sink entries: the plan, fa_decode_num_splits and fa_decode_ws_bytes are
    the twin's."""
    for w in (4096, 0):
        for sinks in (P, None):
            shim = _decode_shim(paged, kv8, w, sinks)
            (cc.decode_paged_argument_checks if paged else cc.decode_argument_checks)(fa_mi355x, shim)


# ---- the Python wrappers -------------------------------------------------------------

def _t(shape, dtype=torch.float16):
    return torch.zeros(shape, dtype=torch.float32).to(dtype)


def _wrapper_calls():
    fa = fa_mi355x
    q4, k = _t((2, 4, 30, 64)), _t((2, 2, 128, 64))
    q3, cu = _t((30, 4, 64)), torch.tensor([0, 10, 30], dtype=torch.int32)
    qd = _t((2, 4, 2, 64))
    table = torch.zeros((2, 2), dtype=torch.int32)
    return [
        lambda **kw: fa.flash_attention_decode(qd, k, k, **kw),
        lambda **kw: fa.flash_attention_decode_paged(qd, k, k, table, **kw),
        lambda **kw: fa.flash_attention_prefill(q4, k, k, **kw),
        lambda **kw: fa.flash_attention_prefill_paged(q4, k, k, table, **kw),
        lambda **kw: fa.flash_attention_prefill_varlen(q3, k, k, cu, **kw),
        lambda **kw: fa.flash_attention_prefill_varlen_paged(q3, k, k, table, cu, **kw),
    ]


def test_wrapper_rejections():
    """sinks is checked in k_scale's wording, before where the tensors live:
    float32, 1-D, [Hq], contiguous, a tensor -> FA_ERR_BAD_SHAPE; its values are
    not looked at; a bad window beside it is still named first."""
    fa = fa_mi355x
    good = torch.zeros(4)
    bad = [
        (torch.zeros(4, dtype=torch.float16), r"got torch.float16 \[4\]"),
        (torch.zeros(4, dtype=torch.float64), r"got torch.float64 \[4\]"),
        (torch.zeros(4, dtype=torch.bfloat16), r"got torch.bfloat16 \[4\]"),
        (torch.zeros(2), r"got torch.float32 \[2\]"),          # [Hkv], not [Hq]
        (torch.zeros(5), r"got torch.float32 \[5\]"),
        (torch.zeros((4, 1)), r"got torch.float32 \[4, 1\]"),
        (torch.zeros((1, 4)), r"got torch.float32 \[1, 4\]"),
        (torch.zeros(()), r"got torch.float32 \[\]"),
        (torch.zeros(8)[::2], r"got torch.float32 \[4\]"),     # not contiguous
        ([0.0] * 4, "got list"),
        (0.5, "got float"),
    ]
    for f in _wrapper_calls():
        for s, got in bad:
            for w in (0, 4):
                with pytest.raises(err, match=r"sinks must be a contiguous float32 \[Hq = 4\] tensor, " + got) as e:
                    f(sinks=s, window=w)
                assert e.value.status == fa.FA_ERR_BAD_SHAPE
        # a bad window is named first, whatever sinks is
        with pytest.raises(err, match=r"window must be >= 0 \(0: no window\), got -1"):
            f(sinks=torch.zeros(5), window=-1)
        with pytest.raises(err, match="a window needs causal=True"):
            f(sinks=torch.zeros(5), window=4, causal=False)
        with pytest.raises(err, match="window must be an int, got float"):
            f(sinks=good, window=1.5)
        # good sinks (any values: NaN and -inf are not looked at): what is left is where the tensors live
        for s in (good, torch.full((4,), NINF), torch.full((4,), float("nan"))):
            for kw in (dict(window=0), dict(window=4), dict(window=0, causal=False)):
                with pytest.raises(err, match="q must be a device tensor") as e:
                    f(sinks=s, **kw)
                assert e.value.status == fa.FA_ERR_NULL_POINTER
        # k_scale's own check comes before sinks' (beside a 16-bit cache: refused outright)
        with pytest.raises(err, match="k_scale / v_scale go with a torch.float8_e4m3fn cache only"):
            f(sinks=torch.zeros(5), k_scale=torch.zeros(2))
        # ... and without sinks nothing changed
        with pytest.raises(err, match="q must be a device tensor"):
            f()


def test_entry_selection():
    """None takes today's path (the plain or the `_win` entry); a tensor takes the
    `_sink` entry with the given window, 0 included."""
    ev = fa_mi355x._entry_variant
    s = torch.zeros(4)
    assert ev(0, None) == ("", ()) and ev(7, None) == ("_win", (7,))
    assert ev(0, s) == ("_sink", (0, s.data_ptr())) and ev(7, s) == ("_sink", (7, s.data_ptr()))


# ---- torch ops -----------------------------------------------------------------------

# the default overloads (and decode_paged.kv8), as the existing tests pin them
PINNED = {
    "decode": "decode(Tensor q, Tensor k_cache, Tensor v_cache, Tensor? kv_lens=None, bool causal=True, "
              "Tensor? k_scale=None, Tensor? v_scale=None) -> Tensor",
    "decode_paged": "decode_paged(Tensor q, Tensor k_pages, Tensor v_pages, Tensor block_table, "
                    "Tensor? kv_lens=None, bool causal=True) -> Tensor",
    "prefill": "prefill(Tensor q, Tensor k_cache, Tensor v_cache, Tensor? kv_lens=None, Tensor? q_lens=None, "
               "bool causal=True, Tensor? k_scale=None, Tensor? v_scale=None) -> Tensor",
    "prefill_paged": "prefill_paged(Tensor q, Tensor k_pages, Tensor v_pages, Tensor block_table, "
                     "Tensor? kv_lens=None, Tensor? q_lens=None, bool causal=True, Tensor? k_scale=None, "
                     "Tensor? v_scale=None) -> Tensor",
    "prefill_varlen": "prefill_varlen(Tensor q, Tensor k_cache, Tensor v_cache, Tensor cu_seqlens_q, "
                      "Tensor? kv_lens=None, bool causal=True, Tensor? k_scale=None, Tensor? v_scale=None) "
                      "-> Tensor",
    "prefill_varlen_paged": "prefill_varlen_paged(Tensor q, Tensor k_pages, Tensor v_pages, "
                            "Tensor block_table, Tensor cu_seqlens_q, Tensor? kv_lens=None, bool causal=True, "
                            "Tensor? k_scale=None, Tensor? v_scale=None) -> Tensor",
}


def test_sinks_ops_and_unchanged_schemas():
    import fa_mi355x.torch_op as top
    from torch._subclasses.fake_tensor import FakeTensorMode

    for name, sig in PINNED.items():
        op = getattr(top, name)
        assert str(op.default._schema) == "fa_mi355x::" + sig, name
        lead = sig[sig.index("(") + 1:sig.index(") ->")].replace(", Tensor? k_scale=None, Tensor? v_scale=None", "")
        win = f"{lead}, Tensor? k_scale=None, Tensor? v_scale=None, int window=0"
        assert str(op.window._schema) == f"fa_mi355x::{name}.window({win}) -> Tensor", name
        # .sinks: the .window overload's arguments, then Tensor? sinks=None
        assert str(op.sinks._schema) == f"fa_mi355x::{name}.sinks({win}, Tensor? sinks=None) -> Tensor", name
        assert op.overloads()[-1] == "sinks" and op.overloads().index("window") < op.overloads().index("sinks")
    assert str(top.decode_paged.kv8._schema).endswith(
        "bool causal=True, Tensor? k_scale=None, Tensor? v_scale=None) -> Tensor")
    q, k = _t((1, 2, 4, 64)), _t((1, 2, 64, 64))
    q3, cu = _t((20, 2, 64)), torch.tensor([0, 20], dtype=torch.int32)
    table = torch.zeros((1, 1), dtype=torch.int32)
    s = torch.zeros(2)
    for name, args in (("decode", (q, k, k)), ("decode_paged", (q, k, k, table)), ("prefill", (q, k, k)),
                       ("prefill_paged", (q, k, k, table)), ("prefill_varlen", (q3, k, k, cu)),
                       ("prefill_varlen_paged", (q3, k, k, table, cu))):
        op = getattr(top, name)
        # which overload a call resolves to shows in the message its CPU kernel raises
        for kw in (dict(sinks=s), dict(sinks=s, window=3), dict(sinks=None)):
            with pytest.raises(ValueError, match=f"fa_mi355x::{name} needs GPU tensors"):
                op(*args, **kw)
        with pytest.raises(ValueError, match=f"fa_mi355x::{name} needs GPU tensors"):
            op(*args, window=3)
        with pytest.raises(ValueError, match=f"{name} needs GPU tensors"):
            op(*args)
        # calls without sinks resolve to the earlier overloads
        for kw, want in ((dict(), "default"), (dict(causal=False), "default"), (dict(window=3), "window"),
                         (dict(sinks=s), "sinks"), (dict(window=3, sinks=s), "sinks")):
            if name == "decode_paged" and want == "default":
                kws = [(kw, "default"), (dict(kw, k_scale=None), "kv8")]
            else:
                kws = [(kw, want)]
            for kk, ww in kws:
                assert _resolved(op, args, kk) == ww, (name, kk)
    with FakeTensorMode():
        fq = torch.empty((2, 8, 300, 128), dtype=torch.bfloat16)
        fd = torch.empty((2, 8, 4, 128), dtype=torch.bfloat16)
        fk = torch.empty((2, 2, 576, 128), dtype=torch.bfloat16)
        ft = torch.empty((2, 9), dtype=torch.int32)
        fp = torch.empty((600, 8, 128), dtype=torch.bfloat16)
        fcu = torch.empty((3,), dtype=torch.int32)
        fs = torch.empty((8,), dtype=torch.float32)
        assert top.decode(fd, fk, fk, sinks=fs).shape == fd.shape
        assert top.decode_paged(fd, fk, fk, ft, window=64, sinks=fs).shape == fd.shape
        assert top.prefill(fq, fk, fk, sinks=fs, window=64).shape == fq.shape
        assert top.prefill(fq, fk, fk, None, None, True, None, None, 64, fs).shape == fq.shape
        assert top.prefill_paged(fq, fk, fk, ft, sinks=fs).shape == fq.shape
        assert top.prefill_varlen(fp, fk, fk, fcu, sinks=fs).shape == fp.shape
        assert top.prefill_varlen_paged(fp, fk, fk, ft, fcu, window=64, sinks=fs).shape == fp.shape
        assert top.prefill(fq, fk, fk, window=64).shape == fq.shape  # .window, as before


def _resolved(packet, args, kwargs):
    """The overload torch's dispatcher resolves the call to."""
    return torch._C._jit_resolve_packet(packet._qualified_op_name, *args, **kwargs)


# ---- compile-time resources ----------------------------------------------------------

FORMS = sr.FORMS
PRE_UNITS = [f"{fam}_sink{form}.hip" for fam in ("fa_prefill", "fa_prefill_varlen") for form in FORMS]
DEC_UNITS = [f"fa_decode_sink{form}.hip" for form in FORMS]


def test_kernel_resource_usage():
    """The siblings' budget holds for every Sinked<> instantiation: no scratch;
    the prefill kernels' one LDS constant; decode's LDS is dynamic (0 static), as
    its siblings'.  Each unit holds the Sinked<> attention kernels only, 4 per
    prefill unit and 12 per decode unit (beside the one-line LSE fill of an
    empty cache, which uses neither scratch nor LDS)."""
    src = open(os.path.join(cc.PKG, "csrc", "fa_prefill_kernel.hpp")).read()
    lds_max = int(re.findall(r"constexpr int kPrefillLdsBytes = (\d+);", src)[0])
    assert lds_max == 65536
    usage = cc.kernel_resource_usage(PRE_UNITS + DEC_UNITS + ["fa_decode_win.hip"])
    for unit, kernels in zip(PRE_UNITS + DEC_UNITS, usage):
        other = [x for x in kernels if "fa_prefill_kernel" not in x[0] and "fa_decode_kernel" not in x[0]]
        assert len(other) == 1 and "fa_sink_fill_lse_kernel" in other[0][0] and other[0][1:] == (0, 0), unit
    for unit, kernels in zip(PRE_UNITS, usage):
        mine = [x for x in kernels if "fa_prefill_kernel" in x[0]]
        assert len(mine) == 4 and all("Sinked" in x[0] and "Windowed" in x[0] for x in mine), \
            (unit, [x[0] for x in kernels])
        assert all(("PrefillPacked" in x[0]) == ("varlen" in unit) for x in mine), unit
        for name, scratch, lds in mine:
            print(f"{unit} {name}: scratch {scratch} LDS {lds}")
            assert scratch == 0 and lds == lds_max, (unit, name, scratch, lds)
    sib = [x for x in usage[-1] if "fa_decode_kernel" in x[0]]
    assert len(sib) == 12 and not any("Sinked" in x[0] for x in sib)
    for unit, kernels in zip(DEC_UNITS, usage[len(PRE_UNITS):-1]):
        mine = [x for x in kernels if "fa_decode_kernel" in x[0]]
        assert len(mine) == 12 and all("Sinked" in x[0] and "Windowed" in x[0] for x in mine), \
            (unit, [x[0] for x in kernels])
        for (name, scratch, lds), (_, s_scratch, s_lds) in zip(mine, sib):
            print(f"{unit} {name}: scratch {scratch} LDS {lds}")
            assert scratch == 0 == s_scratch and lds == s_lds, (unit, name, scratch, lds)
