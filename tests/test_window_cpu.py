"""CPU tests of sliding-window attention (no GPU): the float64 restatement of
the windowed contract against the windowed references at the project's gates,
the interval arithmetic, the 24 fa_*_win_* entries' symbols and argument
statuses (all returned before any launch, so fake pointers suffice), the Python
wrappers' rejections, the `.window` torch ops, the existing ops' schemas, and
the compile-time resource usage of the twelve new units.
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
import keysense_inputs as ks
import window_refs as wr

INT_MAX = cc.INT_MAX
P = ctypes.c_void_p(0x1000)
err = fa_mi355x.FlashAttentionError

FAMILIES = ("fa_decode", "fa_prefill", "fa_prefill_varlen")
ENTRIES = [(fam, paged, kv8, bf16) for fam in FAMILIES for paged in (False, True) for kv8 in (False, True)
           for bf16 in (False, True)]


def _symbol(entry, win=True):
    fam, paged, kv8, bf16 = entry
    return (fam + ("_win" if win else "") + ("_paged" if paged else "") + ("_kv8" if kv8 else "")
            + ("_bf16" if bf16 else "_f16"))


SYMBOLS = [_symbol(e) for e in ENTRIES]


def test_symbols_exported_and_declared():
    assert len(set(SYMBOLS)) == 24
    cc.assert_exported(SYMBOLS)
    header = open(os.path.join(cc.ROOT, "include", "fa_mi355x.h")).read()
    for e in ENTRIES:
        # the twin's argument list with `int window` directly after `causal`
        a, b = (" ".join(re.search(r"\b%s\s*\((.*?)\)" % _symbol(e, w), header, re.S).group(1).split())
                for w in (False, True))
        assert b == a.replace("int causal,", "int causal, int window,"), _symbol(e)


# ---- the interval and the references -------------------------------------------------

def test_interval_arithmetic():
    """[lo, hi) at W in {1, 64, 65, >= len}, with a prefix, and at off_b < 0."""
    # one element: 100 keys of which the chunk's 10 rows are the last (off = 90)
    for w, lo0 in ((1, 90), (64, 27), (65, 26), (100, 0), (4096, 0), (0, 0)):
        lo, hi = wr.interval([100], [10], 1, 12, 128, w)
        assert list(hi[0, :10]) == list(range(91, 101)), w
        assert lo[0, 0] == lo0 and (lo[0, 10:] == -1).all() and (hi[0, 10:] == -1).all(), w
        want = [max(0, 90 + t - w + 1) if w else 0 for t in range(10)]
        assert list(lo[0, :10]) == want, w
        if w:
            assert ((hi - lo)[0, :10] == np.minimum(w, np.arange(91, 101))).all(), w
    # off_b = 3 - 8 < 0: the five leading rows see nothing, row 5 sees key 0 alone
    lo, hi = wr.interval([3], [8], 1, 8, 64, 2)
    assert list(hi[0]) == [0, 0, 0, 0, 0, 1, 2, 3] and list(lo[0]) == [0, 0, 0, 0, 0, 0, 0, 1]
    # decode is the case q_lens = None: pos = len - Sq + t; a length clamped to the capacity
    lo, hi = wr.interval([1000, 5000], None, 2, 4, 1024, 100)
    assert list(hi[0]) == [997, 998, 999, 1000] and list(lo[0]) == [897, 898, 899, 900]
    assert list(hi[1]) == [1021, 1022, 1023, 1024]
    assert wr.block_lo([521, 490], [321, 290], 2, 321, 576, 40) == [[161, 289, 417], [161, 289, 417]]
    assert wr.block_lo([100], [10], 1, 300, 128, 5) == [[86, None, None]]


def _f64_bits(a):
    return a.view(np.float16).astype(np.float64)


@pytest.mark.parametrize("window", [1, 5, 64, 65, 4096])
def test_restatement_against_the_references(window):
    """contract_f64 (its own arithmetic) against the CPU-oracle rows (1e-3), fp32
    torch with the window as a mask (5e-3 is the gate; it is held to 1e-5 here,
    both being exact up to fp32) and the float64 LSE, ragged q_lens, a negative
    off_b included."""
    b, hq, hkv, sq, cap, d = 3, 4, 2, 40, 192, 64
    kv_lens, q_lens = (150, 20, 192), (40, 33, 7)
    q, k, v = dr.inputs(b, hq, hkv, sq, cap, d)
    o, lse, written, smax = wr.contract_f64(_f64_bits(q), _f64_bits(k), _f64_bits(v), kv_lens, q_lens, window,
                                            with_smax=True)
    lo, hi = wr.interval(kv_lens, q_lens, b, sq, cap, window)
    assert np.array_equal(written, hi >= 0)
    assert np.array_equal(np.isneginf(lse[:, 0]) & written, (hi == lo) & written)
    assert np.isneginf(lse[1, :, :13]).all() and np.isfinite(lse[1, :, 13:33]).all()
    ro = wr.oracle_rows(q, k, v, kv_lens, q_lens, window)
    tq, tk, tv = (torch.from_numpy(np.array(a).view(np.int16)).view(torch.float16) for a in (q, k, v))
    to, tl = wr.ref_torch(tq, tk, tv, kv_lens, window, q_lens)
    lref, smax2 = wr.lse_f64(q, k, kv_lens, q_lens, window)
    assert abs(smax - smax2) <= 1e-12
    w3 = np.broadcast_to(written[:, None, :], lse.shape)
    e_or = float(np.abs(_f64_bits(ro)[w3] - o[w3]).max())
    e_to = float(np.abs(to.double().numpy()[w3] - o[w3]).max())
    live = w3 & np.isfinite(lse)
    e_l = float(np.abs(lref[live] - lse[live]).max())
    e_tl = float(np.abs(tl.double().numpy()[live] - lse[live]).max())
    print(f"W={window}: oracle {e_or:.2e} torch {e_to:.2e} lse {e_l:.2e} torch lse {e_tl:.2e}")
    assert e_or <= dr.GATE_F16 and e_to <= 1e-5 and e_l <= 1e-12 and e_tl <= 2.0 ** -10 * smax + 1e-5
    assert np.array_equal(np.isneginf(lref) & w3, np.isneginf(lse) & w3)
    assert not _f64_bits(ro)[~w3].any()


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_negative_score_census_expectation_holds_its_gate(dtype):
    """The hazard test's expectation (Q = +4, K = -4, D = 128: every score
    -181.02; W = 40) against the float64 restatement: the closed form alone
    holds the census gates, so a miss on the GPU is the kernel's."""
    b, hq, hkv, sq, cap, d, w = 1, 2, 1, 70, 256, 128, 40
    kv_lens, q_lens = (230,), (70,)
    q, k, v, counts = wr.census_qkv((b, hq, sq, d), (b, hkv, cap, d), 4.0, -4.0, "stripe", dtype)
    score = wr.census_score(4.0, -4.0, d)
    assert abs(score + 181.0193) < 1e-3
    o, lse, _ = wr.contract_f64(q.double().numpy(), k.double().numpy(), v.double().numpy(), kv_lens, q_lens, w)
    lo, hi = wr.interval(kv_lens, q_lens, b, sq, cap, w)
    assert ((hi - lo) == w).all()
    o16 = torch.from_numpy(o).to(dtype).double()  # the final rounding the gate allows
    wr.check_census(o16, torch.from_numpy(lo)[:, None], torch.from_numpy(hi)[:, None], counts, score,
                    f"restatement {dtype}", lse=torch.from_numpy(lse), dtype=dtype).require()
    assert abs(float(lse[0, 0, 0]) - (score + math.log(w))) < 1e-9
    # and the checker sees one key too many or too few at either edge
    for dlo, dhi in ((1, 0), (-1, 0), (0, -1)):
        bad, _, _ = wr.contract_f64(q.double().numpy(), k.double().numpy(), v.double().numpy(),
                                    (230 + dhi,), q_lens, w - dlo + dhi)
        res = wr.check_census(torch.from_numpy(bad).to(dtype).double(), torch.from_numpy(lo)[:, None],
                              torch.from_numpy(hi)[:, None], counts, score, "moved edge", dtype=dtype)
        assert not res.ok, (dlo, dhi)


def test_windowed_census_reduces_to_keysense_without_a_window():
    counts = ks.census_counts(ks.census_v(300, 64, "stripe"))
    vis = torch.tensor([0, 1, 64, 65, 300])
    o0, l0 = ks.census_expected(counts, vis, 0.25)
    o1, l1 = wr.census_expected(counts, torch.zeros_like(vis), vis, wr.census_score(0.25, 0.25, 64))
    assert torch.equal(o0, o1) and torch.equal(l0, l1)
    o2, _ = wr.census_expected(counts, torch.tensor([10]), torch.tensor([74]), 0.0)
    assert float(o2.sum()) == 1.0 and float(o2.max()) == 1.0 / 64


# ---- the C entries' argument statuses ------------------------------------------------

def _call(entry, q, k, v, o, b, hq, hkv, sq, cap, d, lens=None, ql=None, cu=P, causal=1, window=5, ns=0,
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
        return fn(q, k, v, o, None, b, hq, hkv, sq, *cache, lens, causal, window, ns, ws, wsb, None, *tail)
    second = cu if fam == "fa_prefill_varlen" else ql
    return fn(q, k, v, o, None, b, hq, hkv, sq, *cache, lens, second, causal, window, None, *tail)


@pytest.mark.parametrize("entry", ENTRIES, ids=SYMBOLS)
def test_window_argument_statuses(entry):
    """The window's own statuses and their place in the twin's order: W < 0 with
    the negative counts (before head_dim and before an empty problem's FA_OK),
    W > 0 without causal right after the seqlen_q / total_q check (after
    head_dim, before the page geometry and before an empty problem's FA_OK);
    every other status of the twin arrives as it does there."""
    fa = fa_mi355x
    fam, paged, _, _ = entry
    call = lambda *a, **kw: _call(entry, *a, **kw)  # noqa: E731
    sq = 4 if fam == "fa_decode" else 300
    b = 3
    good = (b, 8, 2, sq, 1024, 128)
    # a good shape is accepted with any W >= 0: what is left is the NULL q
    for w in (0, 1, 64, 4096, INT_MAX):
        assert call(None, P, P, P, *good, window=w) == fa.FA_ERR_NULL_POINTER, w
    assert call(None, P, P, P, *good, window=0, causal=0) == fa.FA_ERR_NULL_POINTER
    # W < 0: with the negative counts
    for w in (-1, -INT_MAX - 1):
        assert call(P, P, P, P, *good, window=w) == fa.FA_ERR_BAD_SHAPE
        assert call(P, P, P, P, b, 8, 2, sq, 1024, 96, window=w) == fa.FA_ERR_BAD_SHAPE
        assert call(None, None, None, None, 0, 8, 2, sq, 1024, 128, window=w, table=None, cu=None) == \
            fa.FA_ERR_BAD_SHAPE
    # W > 0 without causal: after head_dim and seqlen_q, before the page geometry and FA_OK
    assert call(P, P, P, P, *good, window=1, causal=0) == fa.FA_ERR_BAD_SHAPE
    assert call(P, P, P, P, b, 8, 2, sq, 1024, 96, window=1, causal=0) == fa.FA_ERR_UNSUPPORTED_HEAD_DIM
    assert call(None, None, None, None, 0, 8, 2, sq, 1024, 128, window=1, causal=0, table=None, cu=None) == \
        fa.FA_ERR_BAD_SHAPE
    assert call(None, None, None, None, 0, 8, 2, sq, 1024, 128, window=0, causal=0, table=None, cu=None) == \
        fa.FA_OK
    # the twin's table, with a window
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
        assert call(P, P, P, P, 1, 8, 2, 1 << 23, 1024, 128) == fa.FA_ERR_BAD_SHAPE  # seqlen_q * 2 * D
    if paged:
        assert call(P, P, P, P, *good, table=None) == fa.FA_ERR_NULL_POINTER
        for psz in (0, 32, 96, -64, 1, 63, 65):
            assert call(P, P, P, P, *good, psz=psz, mpp=8) == fa.FA_ERR_BAD_SHAPE, psz
        for npages in (0, -1):
            assert call(P, P, P, P, *good, npages=npages) == fa.FA_ERR_BAD_SHAPE
        assert call(P, P, P, P, *good, mpp=-1) == fa.FA_ERR_BAD_SHAPE
        assert call(P, P, P, P, b, 8, 2, sq, 0, 128, psz=64, mpp=2147483520 // 64 + 1) == fa.FA_ERR_BAD_SHAPE
        assert call(P, P, P, P, b, 8, 2, sq, 0, 128, npages=1, psz=1 << 23, mpp=1) == fa.FA_ERR_BAD_SHAPE
        # the page geometry is checked for an empty problem too
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


def _decode_shim(paged, kv8, window):
    """The loaded library with fa_decode[_paged]_f16 / _bf16 bound to the windowed
    entries at a fixed window, for capi_checks' decode tables."""
    lib = fa_mi355x.load_library()
    shim = types.SimpleNamespace(fa_decode_ws_bytes=lib.fa_decode_ws_bytes,
                                 fa_decode_num_splits=lib.fa_decode_num_splits)
    at = 15 if paged else 12  # the arguments up to and including causal

    def bind(fn):
        tail = (None, None) if kv8 else ()
        return lambda *a: fn(*a[:at + 1], window, *a[at + 1:], *tail)

    for ty in ("_f16", "_bf16"):
        name = "fa_decode" + ("_paged" if paged else "") + ty
        setattr(shim, name, bind(getattr(lib, "fa_decode_win" + ("_paged" if paged else "")
                                         + ("_kv8" if kv8 else "") + ty)))
    return shim


@pytest.mark.parametrize("kv8", [False, True], ids=["16bit", "kv8"])
@pytest.mark.parametrize("paged", [False, True], ids=["contig", "paged"])
def test_decode_twins_tables_with_a_window(paged, kv8):
    """capi_checks' whole decode tables (workspace statuses included) hold for
    the windowed entries.  W = 4096 and W = 0: the plan sees the capacities the
    tables use, so the workspace they size is the one the entry asks for."""
    for w in (4096, 0):
        shim = _decode_shim(paged, kv8, w)
        (cc.decode_paged_argument_checks if paged else cc.decode_argument_checks)(fa_mi355x, shim)


def test_decode_window_plan():
    """num_splits = 0 with a window plans from min(cap, 64 ceil((W + Sq - 1) / 64)
    + 64): a short window in a long cache does not split (no workspace asked
    for) where the twin does."""
    fa = fa_mi355x
    lib = fa.load_library()
    assert fa.decode_window_capacity(32768, 1, 4096) == 4096 + 64
    assert fa.decode_window_capacity(32768, 16, 4096) == 4096 + 64 + 64
    assert fa.decode_window_capacity(32768, 1, 1) == 128
    assert fa.decode_window_capacity(1024, 4, 4096) == 1024
    assert fa.decode_window_capacity(1024, 4, 0) == 1024
    assert lib.fa_decode_num_splits(1, 8, 2, 1, 32768, 128) > 1
    assert lib.fa_decode_num_splits(1, 8, 2, 1, fa.decode_window_capacity(32768, 1, 64), 128) == 1
    # (a call that passes every check would launch: only refusals are made here)
    e = ("fa_decode", False, False, False)
    assert _call(e, P, P, P, P, 1, 8, 2, 1, 32768, 128, window=0) == fa.FA_ERR_WORKSPACE
    # W = 4096 in 32k: split, by the plan of the window's capacity: one byte less
    # than fa_decode_ws_bytes at that capacity is refused, and it is less than the twin needs
    ns = lib.fa_decode_num_splits(1, 8, 2, 1, 4160, 128)
    need = lib.fa_decode_ws_bytes(1, 8, 2, 1, 4160, 128, 0)
    assert ns > 1 and need == lib.fa_decode_ws_bytes(1, 8, 2, 1, 32768, 128, ns)
    assert need < lib.fa_decode_ws_bytes(1, 8, 2, 1, 32768, 128, 0)
    assert _call(e, P, P, P, P, 1, 8, 2, 1, 32768, 128, window=4096, ws=P, wsb=need - 1) == \
        fa.FA_ERR_WORKSPACE
    assert _call(e, P, P, P, P, 1, 8, 2, 1, 32768, 128, window=4096) == fa.FA_ERR_WORKSPACE


# ---- the Python wrappers -------------------------------------------------------------

def _t(shape, dtype=torch.float16):
    return torch.zeros(shape, dtype=torch.float32).to(dtype)


def test_wrapper_rejections():
    fa = fa_mi355x
    q4, k = _t((2, 4, 30, 64)), _t((2, 2, 128, 64))
    q3, cu = _t((30, 4, 64)), torch.tensor([0, 10, 30], dtype=torch.int32)
    qd = _t((2, 4, 2, 64))
    table = torch.zeros((2, 2), dtype=torch.int32)
    calls = [
        lambda **kw: fa.flash_attention_decode(qd, k, k, **kw),
        lambda **kw: fa.flash_attention_decode_paged(qd, k, k, table, **kw),
        lambda **kw: fa.flash_attention_prefill(q4, k, k, **kw),
        lambda **kw: fa.flash_attention_prefill_paged(q4, k, k, table, **kw),
        lambda **kw: fa.flash_attention_prefill_varlen(q3, k, k, cu, **kw),
        lambda **kw: fa.flash_attention_prefill_varlen_paged(q3, k, k, table, cu, **kw),
    ]
    for f in calls:
        with pytest.raises(err, match=r"window must be >= 0 \(0: no window\), got -1") as e:
            f(window=-1)
        assert e.value.status == fa.FA_ERR_BAD_SHAPE
        with pytest.raises(err, match="a window needs causal=True") as e:
            f(window=4, causal=False)
        assert e.value.status == fa.FA_ERR_BAD_SHAPE
        for bad, ty in ((1.5, "float"), ("4", "str"), (None, "NoneType"), (True, "bool")):
            with pytest.raises(err, match=f"window must be an int, got {ty}"):
                f(window=bad)
        # a good window: what is left is where the tensors live, as without one
        for w in (0, 4):
            with pytest.raises(err, match="q must be a device tensor"):
                f(window=w)
        with pytest.raises(err, match="q must be a device tensor"):
            f(window=0, causal=False)


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


def test_window_ops_and_unchanged_schemas():
    import fa_mi355x.torch_op as top
    from torch._subclasses.fake_tensor import FakeTensorMode

    for name, sig in PINNED.items():
        op = getattr(top, name)
        assert str(op.default._schema) == "fa_mi355x::" + sig, name
        # .window: the default's arguments, the scales, then int window
        lead = sig[sig.index("(") + 1:sig.index(") ->")].replace(", Tensor? k_scale=None, Tensor? v_scale=None", "")
        want = (f"fa_mi355x::{name}.window({lead}, Tensor? k_scale=None, Tensor? v_scale=None, "
                "int window=0) -> Tensor")
        assert str(op.window._schema) == want, name
    assert str(top.decode_paged.kv8._schema).endswith(
        "bool causal=True, Tensor? k_scale=None, Tensor? v_scale=None) -> Tensor")
    q, k = _t((1, 2, 4, 64)), _t((1, 2, 64, 64))
    q3, cu = _t((20, 2, 64)), torch.tensor([0, 20], dtype=torch.int32)
    table = torch.zeros((1, 1), dtype=torch.int32)
    for name, args in (("decode", (q, k, k)), ("decode_paged", (q, k, k, table)), ("prefill", (q, k, k)),
                       ("prefill_paged", (q, k, k, table)), ("prefill_varlen", (q3, k, k, cu)),
                       ("prefill_varlen_paged", (q3, k, k, table, cu))):
        with pytest.raises(ValueError, match=f"fa_mi355x::{name} needs GPU tensors"):
            getattr(top, name)(*args, window=3)
        with pytest.raises(ValueError, match=f"{name} needs GPU tensors"):
            getattr(top, name)(*args)  # still the default overload
    with FakeTensorMode():
        fq = torch.empty((2, 8, 300, 128), dtype=torch.bfloat16)
        fd = torch.empty((2, 8, 4, 128), dtype=torch.bfloat16)
        fk = torch.empty((2, 2, 576, 128), dtype=torch.bfloat16)
        ft = torch.empty((2, 9), dtype=torch.int32)
        fp = torch.empty((600, 8, 128), dtype=torch.bfloat16)
        fcu = torch.empty((3,), dtype=torch.int32)
        assert top.decode(fd, fk, fk, window=64).shape == fd.shape
        assert top.decode_paged(fd, fk, fk, ft, window=64).shape == fd.shape
        assert top.prefill(fq, fk, fk, window=64).shape == fq.shape
        assert top.prefill(fq, fk, fk, None, None, True, None, None, 64).shape == fq.shape
        assert top.prefill_paged(fq, fk, fk, ft, window=64).shape == fq.shape
        assert top.prefill_varlen(fp, fk, fk, fcu, window=64).shape == fp.shape
        assert top.prefill_varlen_paged(fp, fk, fk, ft, fcu, window=64).shape == fp.shape


# ---- compile-time resources ----------------------------------------------------------

FORMS = ("", "_paged", "_kv8", "_paged_kv8")
PRE_UNITS = [f"{fam}_win{form}.hip" for fam in ("fa_prefill", "fa_prefill_varlen") for form in FORMS]
DEC_UNITS = [f"fa_decode_win{form}.hip" for form in FORMS]


def test_kernel_resource_usage():
    """The siblings' budget holds for every windowed instantiation: no scratch;
    the prefill kernels' one LDS constant; decode's LDS is dynamic (0 static),
    as its siblings'.  Each unit holds the Windowed<> kernels only."""
    src = open(os.path.join(cc.PKG, "csrc", "fa_prefill_kernel.hpp")).read()
    lds_max = int(re.findall(r"constexpr int kPrefillLdsBytes = (\d+);", src)[0])
    assert lds_max == 65536
    usage = cc.kernel_resource_usage(PRE_UNITS + DEC_UNITS + ["fa_decode.hip"])
    for unit, kernels in zip(PRE_UNITS, usage):
        mine = [x for x in kernels if "fa_prefill_kernel" in x[0]]
        assert len(mine) == 4 and all("Windowed" in x[0] for x in mine), (unit, [x[0] for x in kernels])
        assert all(("PrefillPacked" in x[0]) == ("varlen" in unit) for x in mine), unit
        for name, scratch, lds in mine:
            print(f"{unit} {name}: scratch {scratch} LDS {lds}")
            assert scratch == 0 and lds == lds_max, (unit, name, scratch, lds)
    sib = [x for x in usage[-1] if "fa_decode_kernel" in x[0]]
    assert len(sib) == 12
    for unit, kernels in zip(DEC_UNITS, usage[len(PRE_UNITS):-1]):
        mine = [x for x in kernels if "fa_decode_kernel" in x[0]]
        assert len(mine) == 12 and all("Windowed" in x[0] for x in mine), (unit, [x[0] for x in kernels])
        for (name, scratch, lds), (_, s_scratch, s_lds) in zip(mine, sib):
            print(f"{unit} {name}: scratch {scratch} LDS {lds}")
            assert scratch == 0 == s_scratch and lds == s_lds, (unit, name, scratch, lds)
