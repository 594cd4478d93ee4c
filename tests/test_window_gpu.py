"""GPU tests of sliding-window attention: the fa_prefill_win_*,
fa_prefill_varlen_win_* and fa_decode_win_* entries through the `window=`
keyword of the six Python functions, over the four cache forms.

References, gates and the closed-form inputs are tests/window_refs.py's (the
project's: census at keysense_inputs' gates, needle 1e-3, fp16 O 1e-3 against
the CPU oracle, bf16 O 5e-3 against fp32 torch, LSE 2^-10 max|score| + 1e-5);
tests/test_window_cpu.py holds them against a float64 restatement.  The other
cache forms are held to the contiguous 16-bit result BIT FOR BIT (paged on the
gathered cache; FP8 with unit scales on values exact in E4M3), so every check
made on the contiguous result is made on all four.

Prefill runs at prefill_refs' key-sensitivity shape (B=2, Hq=8, Hkv=2, Sq=321
behind 200 keys, cap 576, q_lens (321, 290)): three query blocks, and tlo > 0
for the later ones once W is small.  Decode runs at B=3, Hq=8, Hkv=2, cap
1024, lens (1, 130, 1000).
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
import window_refs as wr

pytestmark = pytest.mark.gpu

DEV = "cuda"
FP8 = torch.float8_e4m3fn
PAD8 = 0x7f  # the E4M3 NaN
F16, BF16 = torch.float16, torch.bfloat16
K_SCALE = (2.0 ** -6, 2.0 ** -3)
V_SCALE = (2.0 ** -4, 2.0 ** -8)

prefill = fa_mi355x.flash_attention_prefill
prefill_paged = fa_mi355x.flash_attention_prefill_paged
prefill_varlen = fa_mi355x.flash_attention_prefill_varlen
prefill_varlen_paged = fa_mi355x.flash_attention_prefill_varlen_paged
decode = fa_mi355x.flash_attention_decode
decode_paged = fa_mi355x.flash_attention_decode_paged

B, HQ, HKV, SQ, CAP = pr.KS_B, pr.KS_HQ, pr.KS_HKV, pr.KS_SQ, pr.KS_CAP
Q_LENS, KV_LENS = pr.KS_Q_LENS, pr.KS_KV_LENS
WINDOWS = [1, 17, 63, 64, 65, 128, 130, 200, 1000]  # the last: >= every length
# (form, page size): page 256 with W = 130 gives a tlo that is no page multiple
FORMS = [("paged", 64), ("paged", 128), ("paged", 256), ("contig_kv8", 0), ("paged_kv8", 128),
         ("paged_kv8", 256)]


def _lens(vals):
    return None if vals is None else dr.lens(vals)


def _scale_t(vals):
    return torch.tensor(list(vals), dtype=torch.float32, device=DEV)


def _nan_rows(rows):
    if rows.element_size() == 1:
        rows.view(torch.uint8).fill_(PAD8)
    else:
        rows.view(torch.int16).fill_(dr.NAN_BITS)


def _pad(t, lens, cap_to=None, below=None):
    """A copy with NaN bits (PAD8 in an FP8 cache) in the rows at or past each
    length (and, `below`, in the rows under below[b]), the capacity grown to
    `cap_to` rows of the same."""
    if cap_to is not None and cap_to > t.shape[2]:
        big = torch.empty(t.shape[:2] + (cap_to,) + t.shape[3:], dtype=t.dtype, device=t.device)
        big[:, :, :t.shape[2]] = t
        t = big
    else:
        t = t.clone()
    for i, n in enumerate(lens):
        _nan_rows(t[i, :, min(int(n), t.shape[2]):])
        if below is not None:
            _nan_rows(t[i, :, :int(below[i])])
    return t


def _paginate(k, v, page_size, lens, below=None, **kw):
    """dr.paginate of a cache grown to a multiple of the page size.  below: rows
    under below[b] are NaN, and the table entries of pages lying wholly under
    it point at one in-pool page that holds nothing but NaN."""
    cap = -(-k.shape[2] // page_size) * page_size
    k, v = _pad(k, lens, cap, below), _pad(v, lens, cap, below)
    one = k.dtype is FP8
    if one:
        k, v = k.view(torch.uint8), v.view(torch.uint8)
    kp, vp, table = dr.paginate(k, v, page_size, lens, **kw)
    if below is not None:
        used = set(int(x) for bi, n in enumerate(lens) for x in table[bi, :-(-int(n) // page_size)])
        spare = [p for p in range(kp.shape[0]) if p not in used]
        assert spare and bool(torch.isnan(kp[spare[0]].view(FP8 if one else k.dtype).float()).all())
        for bi, lo in enumerate(below):
            table[bi, :int(lo) // page_size] = spare[0]
    return (kp.view(FP8), vp.view(FP8), table) if one else (kp, vp, table)


def _prefill_form(form, ps, q, k, v, kv_lens, q_lens, window, scales=None, below=None, seed=1):
    """(O, LSE) of one cache form.  k, v: the clean 16-bit caches; a kv8 form
    with scales=None reads their exact E4M3 conversion at unit scales,
    otherwise scales = (k8, v8, k_scale, v_scale)."""
    tl, ql = _lens(kv_lens), _lens(q_lens)
    sc = {}
    if form.endswith("kv8"):
        if scales is None:
            k8, v8 = k.to(FP8), v.to(FP8)
            assert torch.equal(k8.to(k.dtype), k) and torch.equal(v8.to(v.dtype), v)
            k, v = k8, v8
        else:
            k, v = scales[0], scales[1]
            sc = dict(k_scale=scales[2], v_scale=scales[3])
    if form.startswith("paged"):
        kp, vp, table = _paginate(k, v, ps, kv_lens, below, seed=seed + ps)
        return prefill_paged(q, kp, vp, table, tl, ql, return_lse=True, window=window, **sc)
    return prefill(q, _pad(k, kv_lens, None, below), _pad(v, kv_lens, None, below), tl, ql, return_lse=True,
                   window=window, **sc)


def _same_rows(a, b, n):
    return all(torch.equal(a[0][bi, :, :nb], b[0][bi, :, :nb]) and torch.equal(a[1][bi, :, :nb], b[1][bi, :, :nb])
               for bi, nb in enumerate(n))


def _all_forms_equal(base, q, k, v, kv_lens, q_lens, window, what, forms=FORMS):
    for form, ps in forms:
        got = _prefill_form(form, ps, q, k, v, kv_lens, q_lens, window)
        assert _same_rows(got, base, pr.n_rows(q_lens, q.shape[0], q.shape[2])), f"{what} {form} page={ps}"


def _interval_t(kv_lens, q_lens, b, sq, cap, window):
    lo, hi = wr.interval(kv_lens, q_lens, b, sq, cap, window)
    return torch.from_numpy(lo)[:, None, :], torch.from_numpy(hi)[:, None, :]


def _check_census(o, lse, counts, kv_lens, q_lens, cap, window, score, what):
    b, _, sq, _ = o.shape
    lo, hi = _interval_t(kv_lens, q_lens, b, sq, cap, window)
    for bi, n in enumerate(pr.n_rows(q_lens, b, sq)):
        if n:
            wr.check_census(o[bi, :, :n], lo[bi, :, :n], hi[bi, :, :n], counts, score, f"{what} b={bi}",
                            lse=lse[bi, :, :n]).require()


# ---- prefill: census, needle ---------------------------------------------------------

@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("d", [128, 64])
@pytest.mark.parametrize("dtype", dr.DTYPES)
def test_prefill_census(dtype, d, window):
    """Who was counted: both levels, both layouts, against the windowed
    expectation; every other cache form equals the contiguous result bit for
    bit (paged at page sizes 64, 128 and 256)."""
    for level in ks.LEVELS:
        for layout in ks.census_layouts(CAP, d):
            q, k, v, counts = pr.ks_census(level, layout, d, dtype, DEV)
            base = _prefill_form("contig", 0, q, k, v, KV_LENS, Q_LENS, window)
            what = f"census {dr.name(dtype)} d={d} W={window} level={level} {layout}"
            _check_census(*base, counts, KV_LENS, Q_LENS, CAP, window, wr.census_score(level, level, d), what)
            if layout == "stripe":
                _all_forms_equal(base, q, k, v, KV_LENS, Q_LENS, window, what)


@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("d", [128, 64])
@pytest.mark.parametrize("dtype", dr.DTYPES)
def test_prefill_needle_at_both_ends(dtype, d, window):
    """Who was read: the target at the row's first visible key (lo) and at its
    last (pos): both ends of the window are read, and nothing beyond outweighs
    them."""
    lo, hi = wr.interval(KV_LENS, Q_LENS, B, SQ, CAP, window)
    k, v = ks.needle_kv((B, HKV), CAP, d, 7, dtype, DEV)
    for end, tgt in (("lo", lo), ("pos", hi - 1)):
        pi = np.where(hi > lo, tgt, 0)                       # rows t >= n_b (not compared): key 0
        pi = torch.from_numpy(np.broadcast_to(pi[:, None, :], (B, HQ, SQ)).copy())
        q = ks.needle_q(k, pi, HQ // HKV)
        want = ks.needle_expected(v, pi, HQ // HKV)
        base = _prefill_form("contig", 0, q, k, v, KV_LENS, Q_LENS, window)
        lref = torch.from_numpy(wr.lse_f64(q, k, KV_LENS, Q_LENS, window)[0])
        what = f"needle {end} {dr.name(dtype)} d={d} W={window}"
        for bi, n in enumerate(Q_LENS):
            ks.check_needle(base[0][bi, :, :n], want[bi, :, :n], pi[bi, :, :n], f"{what} b={bi}",
                            lse=base[1][bi, :, :n], lse_ref=lref[bi, :, :n], d=d).require()
        _all_forms_equal(base, q, k, v, KV_LENS, Q_LENS, window, what, FORMS[2:4])


# ---- prefill: random inputs against the references ------------------------------------

def _quant(x, scale):
    s = _scale_t(scale)[None, :, None, None]
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
    return host, (tq, kd.to(dtype), vd.to(dtype)), (k8, v8, _scale_t(K_SCALE), _scale_t(V_SCALE))


@functools.lru_cache(maxsize=None)
def _refs(b, hq, hkv, sq, cap, d, dtype, kv8, kv_lens, q_lens, window):
    host, clean, _ = _inputs(b, hq, hkv, sq, cap, d, dtype, kv8)
    return wr.refs(host, clean, kv_lens, q_lens, window, dtype)


@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("d", [128, 64])
@pytest.mark.parametrize("dtype", dr.DTYPES)
def test_prefill_random_inputs_against_the_references(dtype, d, window):
    """The project's gates on random inputs; paged equals contiguous on the
    gathered cache bit for bit."""
    _, (q, k, v), _ = _inputs(B, HQ, HKV, SQ, CAP, d, dtype, False)
    refs = _refs(B, HQ, HKV, SQ, CAP, d, dtype, False, KV_LENS, Q_LENS, window)
    base = _prefill_form("contig", 0, q, k, v, KV_LENS, Q_LENS, window)
    what = f"random {dr.name(dtype)} d={d} W={window}"
    pr.check(*base, refs, Q_LENS, dtype, what)
    _all_forms_equal(base, q, k, v, KV_LENS, Q_LENS, window, what, FORMS[:3])


@pytest.mark.parametrize("window", [65, 130])
@pytest.mark.parametrize("d", [128, 64])
@pytest.mark.parametrize("dtype", dr.DTYPES)
def test_prefill_fp8_cache_with_scales_against_the_references(dtype, d, window):
    """An FP8 cache with non-unit scales: the references read the dequantised
    cache; paged FP8 equals contiguous FP8 bit for bit."""
    _, (q, k, v), sc = _inputs(B, HQ, HKV, SQ, CAP, d, dtype, True)
    refs = _refs(B, HQ, HKV, SQ, CAP, d, dtype, True, KV_LENS, Q_LENS, window)
    base = _prefill_form("contig_kv8", 0, q, k, v, KV_LENS, Q_LENS, window, sc)
    pr.check(*base, refs, Q_LENS, dtype, f"fp8 {dr.name(dtype)} d={d} W={window}")
    for ps in (128, 256):
        got = _prefill_form("paged_kv8", ps, q, k, v, KV_LENS, Q_LENS, window, sc)
        assert _same_rows(got, base, Q_LENS), ps


# ---- prefill: bit identities ---------------------------------------------------------

@pytest.mark.parametrize("form,ps", [("contig", 0)] + FORMS[2:5])
@pytest.mark.parametrize("dtype", dr.DTYPES)
def test_prefill_wide_window_and_window_zero_equal_the_plain_entry(dtype, form, ps):
    """W >= every len_b gives the entry without a window, O and LSE, bit for
    bit (the per-row reference is the plain one when every row's first tile is
    tile 0); window=0 is that entry."""
    for d in (128, 64):
        _, (q, k, v), _ = _inputs(B, HQ, HKV, SQ, CAP, d, dtype, False)
        k, v = k.to(FP8).to(dtype), v.to(FP8).to(dtype)  # exact in E4M3 for the kv8 forms
        # (321, 290) behind 200; and lengths shorter than the chunk (off_b < 0)
        for kv_lens in (KV_LENS, (300, 100)):
            plain = _prefill_form(form, ps, q, k, v, kv_lens, Q_LENS, 0)
            for w in (max(kv_lens), CAP, 4096, 2 ** 31 - 1):
                got = _prefill_form(form, ps, q, k, v, kv_lens, Q_LENS, w)
                assert _same_rows(got, plain, Q_LENS), (d, kv_lens, w)


# ---- the C entries with window = 0, causal or not, against their twins ------------------

def _c_entry(fam, paged, win, q, k, v, o, lse, b, hq, hkv, sq, table, kv_lens, second, causal, ns=1, ws=None):
    """One call of fa_<fam>[_win][_paged]_<dtype> through ctypes (win: None = the
    twin without a window, else the window).  second: q_lens / cu_seqlens_q."""
    lib = fa_mi355x.load_library()
    fn = getattr(lib, fam + ("" if win is None else "_win") + ("_paged" if paged else "")
                 + ("_bf16" if q.dtype is BF16 else "_f16"))
    d = q.shape[-1]
    cache = (d, k.shape[0], k.shape[2], table.data_ptr(), table.shape[1]) if paged else (k.shape[2], d)
    w = () if win is None else (win,)
    st = torch.cuda.current_stream().cuda_stream
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    if fam == "fa_decode":
        rc = fn(ptr(q), ptr(k), ptr(v), ptr(o), ptr(lse), b, hq, hkv, sq, *cache, ptr(kv_lens), causal, *w, ns,
                ptr(ws), 0 if ws is None else ws.numel(), st)
    else:
        rc = fn(ptr(q), ptr(k), ptr(v), ptr(o), ptr(lse), b, hq, hkv, sq, *cache, ptr(kv_lens), ptr(second),
                causal, *w, st)
    assert rc == 0, (fam, paged, win, causal, rc)


@pytest.mark.parametrize("paged", [False, True], ids=["contig", "paged"])
@pytest.mark.parametrize("fam", ["fa_prefill", "fa_prefill_varlen", "fa_decode"])
@pytest.mark.parametrize("dtype", dr.DTYPES)
def test_c_entries_with_window_zero_equal_their_twins(dtype, fam, paged):
    """A `_win` entry called with window = 0 computes what its twin computes,
    O and LSE bit for bit, with causal = 1 and with causal = 0 (the one
    combination without causal the entries accept; the Python functions never
    make it, they call the twin)."""
    d = 128
    if fam == "fa_decode":
        b, sq, cap, kv_lens, n = DB, 4, DCAP, DLENS, None
    else:
        b, sq, cap, kv_lens, n = B, SQ, CAP, KV_LENS, Q_LENS
    _, (q, k, v), _ = _inputs(b, HQ, HKV, sq, cap, d, dtype, False)
    table = None
    if paged:
        k, v, table = _paginate(k, v, 128, kv_lens, seed=4)
    else:
        k, v = _pad(k, kv_lens), _pad(v, kv_lens)
    tl = _lens(kv_lens)
    if fam == "fa_prefill_varlen":
        cu = vr.cu_of(n)
        q = vr.pack(q, n, total=cu[-1] + 5, fill=dr.NAN_BITS)
        second, rows, lse_shape = _lens(cu), q.shape[0], (HQ, q.shape[0])
        own = torch.from_numpy(vr.owned_rows(cu, rows)).to(DEV)
    else:
        second, rows, lse_shape = _lens(n), sq, (b, HQ, sq)
    ws = torch.zeros(1 << 22, dtype=torch.uint8, device=DEV) if fam == "fa_decode" else None
    for causal in (1, 0):
        for ns in ((1, 3) if fam == "fa_decode" else (1,)):
            res = []
            for win in (None, 0):
                o = dr.nan_fill(torch.empty_like(q))
                lse = torch.full(lse_shape, float("nan"), dtype=torch.float32, device=DEV)
                _c_entry(fam, paged, win, q, k, v, o, lse, b, HQ, HKV, rows, table, tl, second, causal, ns, ws)
                res.append((o, lse))
            torch.cuda.synchronize()
            what = (fam, paged, causal, ns)
            if fam == "fa_prefill_varlen":
                assert torch.equal(res[0][0][own], res[1][0][own]) and \
                    torch.equal(res[0][1][:, own], res[1][1][:, own]), what
                assert bool(torch.isfinite(res[1][0][own].float()).all()), what
            elif fam == "fa_prefill":
                assert _same_rows(res[0], res[1], n), what
                assert all(bool(torch.isfinite(res[1][1][bi, :, :nb]).all()) for bi, nb in enumerate(n)), what
            else:
                assert dr.same(res[0], res[1]), what


# ---- prefill: the per-row reference ---------------------------------------------------

@pytest.mark.parametrize("dtype", dr.DTYPES)
def test_prefill_rows_whose_first_tiles_are_masked_keep_their_mass(dtype):
    """Q = +4, K = -4 at D = 128: every score is -181.02 (2^-261 against a
    reference left at zero).  With W = 40 the later rows of a 128-row block see
    nothing in the tiles their wave starts with.  Every row of every block must
    count its 40 keys: O is the plain windowed census, LSE = -181.02 + log n.
    (On a reference set once per wave the rows below the first lose all of P:
    O = 0, LSE = -inf.)"""
    d, w = 128, 40
    q, k, v, counts = wr.census_qkv((B, HQ, SQ, d), (B, HKV, CAP, d), 4.0, -4.0, "stripe", dtype, DEV)
    base = _prefill_form("contig", 0, q, k, v, KV_LENS, Q_LENS, w)
    what = f"negative-score census {dr.name(dtype)} W={w}"
    _check_census(*base, counts, KV_LENS, Q_LENS, CAP, w, wr.census_score(4.0, -4.0, d), what)
    assert bool(torch.isfinite(base[1][0]).all())
    _all_forms_equal(base, q, k, v, KV_LENS, Q_LENS, w, what)
    # ... and with leading rows that see nothing at all (off_b < 0)
    short = (300, 100)
    got = _prefill_form("contig", 0, q, k, v, short, Q_LENS, w)
    _check_census(*got, counts, short, Q_LENS, CAP, w, wr.census_score(4.0, -4.0, d), what + " short")


# ---- prefill: what is never read ------------------------------------------------------

@pytest.mark.parametrize("window", [17, 64, 130])
@pytest.mark.parametrize("dtype", dr.DTYPES)
def test_prefill_rows_and_pages_below_the_window_are_never_read(dtype, window):
    """NaN in every cache row below a query block's lo (and past len), and, in
    the paged forms, the table entries of pages wholly below it pointed at an
    in-pool page of NaN: the block's rows equal the clean run bit for bit.  A
    block is run as a chunk of its own (the rows from q0 on, the same kv_lens):
    the same tile sequences, so the same bits, and one lo per call."""
    d = 128
    _, (q, k, v), _ = _inputs(B, HQ, HKV, SQ, CAP, d, dtype, False)
    k, v = k.to(FP8).to(dtype), v.to(FP8).to(dtype)
    clean = _prefill_form("contig", 0, q, k, v, KV_LENS, Q_LENS, window)
    for q0 in (0, 128, 256):
        ql = tuple(n - q0 for n in Q_LENS)
        lo = [max(0, ln - n + q0 - window + 1) for ln, n in zip(KV_LENS, Q_LENS)]
        assert wr.block_lo(KV_LENS, Q_LENS, B, SQ, CAP, window)[0][q0 // 128] == lo[0] and min(lo) > 64
        qc = q[:, :, q0:].contiguous()
        want = (clean[0][:, :, q0:], clean[1][:, :, q0:])
        for form, ps in [("contig", 0)] + FORMS:
            got = _prefill_form(form, ps, qc, k, v, KV_LENS, ql, window, below=lo)
            assert _same_rows(got, want, ql), (q0, form, ps)
            # (q0 = 0 is the whole chunk in one launch: three blocks over a cache
            # poisoned below the smallest lo, the first block's)


# ---- prefill: graph -------------------------------------------------------------------

def test_prefill_window_graph_follows_rewritten_lengths():
    d, w = 128, 65
    _, (q, k, v), _ = _inputs(B, HQ, HKV, SQ, CAP, d, F16, False)
    kp, vp, table = _paginate(k, v, 128, (CAP, CAP), seed=3)
    tl, ql = _lens(KV_LENS), _lens(Q_LENS)
    out = torch.empty_like(q)
    lse = torch.empty((B, HQ, SQ), dtype=torch.float32, device=DEV)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        prefill_paged(q, kp, vp, table, tl, ql, window=w)  # warm-up outside the capture
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            o2, l2 = prefill_paged(q, kp, vp, table, tl, ql, out=out, return_lse=True, window=w)
    torch.cuda.current_stream().wait_stream(stream)
    for kv_lens, q_lens in ((KV_LENS, Q_LENS), ((500, 77), (300, 40))):
        tl.copy_(_lens(kv_lens))
        ql.copy_(_lens(q_lens))
        graph.replay()
        torch.cuda.synchronize()
        want = prefill_paged(q, kp, vp, table, _lens(kv_lens), _lens(q_lens), return_lse=True, window=w)
        assert _same_rows((o2, l2), want, q_lens), kv_lens
        refs = _refs(B, HQ, HKV, SQ, CAP, d, F16, False, kv_lens, q_lens, w)
        pr.check(o2, l2, refs, q_lens, F16, f"graph {kv_lens}")


# ---- packed ---------------------------------------------------------------------------

PB, PT = 5, 600
PN = (0, 1, 127, 128, 321)
PPREFIX = (0, 200, 0, 70, 200)
PKV = tuple(p + n for p, n in zip(PPREFIX, PN))
PCU = vr.cu_of(PN)


@pytest.mark.parametrize("window", [1, 100, 1000])
@pytest.mark.parametrize("dtype", dr.DTYPES)
def test_packed_equals_padded_and_holds_the_gates(dtype, window):
    """varlen_refs' packed shape: sequences shorter than W = 100 (1, 127 keys)
    and longer (198, 521) in one batch, an empty one, a tail of unowned rows.
    Rows t < n_b equal the padded windowed entry bit for bit in all four
    forms, and the contiguous result holds the references' gates."""
    d, smax = 128, max(PN)
    _, (q, k, v), _ = _inputs(PB, HQ, HKV, smax, CAP, d, dtype, False)
    k, v = k.to(FP8).to(dtype), v.to(FP8).to(dtype)
    qp = vr.pack(q, PN, total=PT, fill=dr.NAN_BITS)
    tl, tcu = _lens(PKV), _lens(PCU)
    for form, ps in [("contig", 0), ("paged", 128), ("contig_kv8", 0), ("paged_kv8", 256)]:
        want = _prefill_form(form, ps, q, k, v, PKV, PN, window)
        kk, vv = (k.to(FP8), v.to(FP8)) if form.endswith("kv8") else (k, v)
        if form.startswith("paged"):
            kp, vp, table = _paginate(kk, vv, ps, PKV, seed=1 + ps)
            got = prefill_varlen_paged(qp, kp, vp, table, tcu, tl, return_lse=True, window=window)
        else:
            got = prefill_varlen(qp, _pad(kk, PKV), _pad(vv, PKV), tcu, tl, return_lse=True, window=window)
        got = (vr.unpack(got[0], PCU, smax), vr.unpack(got[1], PCU, smax, fill=float("-inf")))
        assert _same_rows(got, want, PN), (form, ps)
        if form == "contig":
            lo, hi = wr.interval(PKV, PN, PB, smax, CAP, window)
            refs = wr.refs(None, (q, k, v), PKV, PN, window, BF16)  # fp32 torch for both types
            for bi, n in enumerate(PN):
                if n:
                    err = float((got[0][bi, :, :n].float() - refs[0][bi, :, :n]).abs().max())
                    assert err <= (dr.GATE_F16 if dtype is F16 else dr.GATE_BF16), (bi, err)
                    dr.check_lse(got[1][bi:bi + 1, :, :n], refs[1][bi:bi + 1, :, :n], refs[2], f"packed b={bi}")
    # T = 0: nothing to do
    e = prefill_varlen(qp[:0], k, v, _lens([0] * (PB + 1)), tl, return_lse=True, window=window)
    assert e[0].shape == (0, HQ, d) and e[1].shape == (HQ, 0)


# ---- decode ---------------------------------------------------------------------------

DB, DCAP = 3, 1024
DLENS = (1, 130, 1000)
DWINDOWS = [1, 5, 64, 100, 4096]
SPLITS = (1, 3, 8, 0)  # 8 exceeds a short window's tile count: pieces with an empty range
DFORMS = [("paged", 64), ("paged", 256), ("contig_kv8", 0), ("paged_kv8", 128)]


def _decode_form(form, ps, q, k, v, lens, window, ns, scales=None, below=None):
    tl = _lens(lens)
    sc = {}
    if form.endswith("kv8"):
        if scales is None:
            k8, v8 = k.to(FP8), v.to(FP8)
            assert torch.equal(k8.to(k.dtype), k) and torch.equal(v8.to(v.dtype), v)
            k, v = k8, v8
        else:
            k, v = scales[0], scales[1]
            sc = dict(k_scale=scales[2], v_scale=scales[3])
    if form.startswith("paged"):
        kp, vp, table = _paginate(k, v, ps, lens, below, seed=2 + ps)
        return decode_paged(q, kp, vp, table, tl, return_lse=True, num_splits=ns, window=window, **sc)
    return decode(q, _pad(k, lens, None, below), _pad(v, lens, None, below), tl, return_lse=True,
                  num_splits=ns, window=window, **sc)


def _decode_forms_equal(base, q, k, v, lens, window, ns, what):
    for form, ps in DFORMS:
        got = _decode_form(form, ps, q, k, v, lens, window, ns)
        assert dr.same(got, base), f"{what} {form} page={ps}"


@pytest.mark.parametrize("window", DWINDOWS)
@pytest.mark.parametrize("sq", [1, 4, 16])
@pytest.mark.parametrize("dtype", dr.DTYPES)
def test_decode_census_and_needle(dtype, sq, window):
    """Census (both levels, both layouts) and the needle at both ends of the
    window, at every num_splits; the other forms equal the contiguous result
    bit for bit at the same num_splits (the FP8 forms on these inputs, whose
    score sums are exact: the FP8 decode kernel adds a score's products in
    another order than the 16-bit one).  D = 128, and 64 at the plan's own
    split and one forced."""
    lo, hi = _interval_t(DLENS, None, DB, sq, DCAP, window)
    for d, splits in ((128, SPLITS), (64, (0, 3))):
        kn, vn = ks.needle_kv((DB, HKV), DCAP, d, 11, dtype, DEV)
        for ns in splits:
            what = f"decode {dr.name(dtype)} d={d} Sq={sq} W={window} ns={ns}"
            for level in ks.LEVELS:
                for layout in ks.census_layouts(DCAP, d):
                    q, k, v, counts = ks.census_qkv((DB, HQ, sq, d), (DB, HKV, DCAP, d), level, layout, dtype,
                                                    DEV)
                    base = _decode_form("contig", 0, q, k, v, DLENS, window, ns)
                    wr.check_census(base[0], lo, hi, counts, wr.census_score(level, level, d),
                                    f"census level={level} {layout} " + what, lse=base[1]).require()
                    if layout == "stripe":
                        _decode_forms_equal(base, q, k, v, DLENS, window, ns, what)
            for end, tgt in (("lo", lo), ("pos", hi - 1)):
                pi = torch.where(hi > lo, tgt, torch.full_like(tgt, -1)).expand(DB, HQ, sq).contiguous()
                qn = ks.needle_q(kn, pi, HQ // HKV)
                got = _decode_form("contig", 0, qn, kn, vn, DLENS, window, ns)
                lref = torch.from_numpy(wr.lse_f64(qn, kn, DLENS, None, window)[0])
                ks.check_needle(got[0], ks.needle_expected(vn, pi, HQ // HKV), pi, f"needle {end} " + what,
                                lse=got[1], lse_ref=lref, d=d).require()
        assert dr.ws_counters_zero()


@pytest.mark.parametrize("window", DWINDOWS)
@pytest.mark.parametrize("sq", [1, 4, 16])
@pytest.mark.parametrize("dtype", dr.DTYPES)
def test_decode_random_inputs_against_the_references(dtype, sq, window):
    """The project's decode gates; W >= len equals the entry without a window
    at the same num_splits bit for bit; an FP8 cache with scales holds the
    gates on the dequantised cache."""
    d = 128
    _, (q, k, v), _ = _inputs(DB, HQ, HKV, sq, DCAP, d, dtype, False)
    refs = _refs(DB, HQ, HKV, sq, DCAP, d, dtype, False, DLENS, None, window)
    for ns in SPLITS:
        base = _decode_form("contig", 0, q, k, v, DLENS, window, ns)
        dr.check(*base, refs, dtype, f"decode random {dr.name(dtype)} Sq={sq} W={window} ns={ns}")
        got = _decode_form("paged", 128, q, k, v, DLENS, window, ns)
        assert dr.same(got, base), ns
        if window >= max(DLENS):
            assert dr.same(base, _decode_form("contig", 0, q, k, v, DLENS, 0, ns)), ns
            assert dr.same(got, _decode_form("paged", 128, q, k, v, DLENS, 0, ns)), ns
    _, (q8, k8, v8), sc = _inputs(DB, HQ, HKV, sq, DCAP, d, dtype, True)
    refs8 = _refs(DB, HQ, HKV, sq, DCAP, d, dtype, True, DLENS, None, window)
    for form, ps in (("contig_kv8", 0), ("paged_kv8", 128)):
        got = _decode_form(form, ps, q8, k8, v8, DLENS, window, 0, sc)
        dr.check(*got, refs8, dtype, f"decode fp8 {form} {dr.name(dtype)} Sq={sq} W={window}")


@pytest.mark.parametrize("dtype", dr.DTYPES)
def test_decode_rows_masked_in_the_first_tile_keep_their_mass(dtype):
    """(len - Sq + 1 - W) mod 64 = 63 (len 1000, Sq 16, W 26: lo = 959): rows 1 to
    15 see nothing in the first tile.  Negative-score census (Q = +4, K = -4:
    every score -181.02): every row counts its keys, at every num_splits."""
    d, sq, w = 128, 16, 26
    assert (DLENS[2] - sq + 1 - w) % 64 == 63
    q, k, v, counts = wr.census_qkv((DB, HQ, sq, d), (DB, HKV, DCAP, d), 4.0, -4.0, "stripe", dtype, DEV)
    lo, hi = _interval_t(DLENS, None, DB, sq, DCAP, w)
    for ns in SPLITS:
        base = _decode_form("contig", 0, q, k, v, DLENS, w, ns)
        what = f"decode negative-score census {dr.name(dtype)} ns={ns}"
        wr.check_census(base[0], lo, hi, counts, wr.census_score(4.0, -4.0, d), what, lse=base[1]).require()
        _decode_forms_equal(base, q, k, v, DLENS, w, ns, what)


@pytest.mark.parametrize("window", [5, 100])
@pytest.mark.parametrize("dtype", dr.DTYPES)
def test_decode_rows_and_pages_below_the_window_are_never_read(dtype, window):
    """NaN in the cache rows below row 0's lower bound (and past len), the table
    entries of pages wholly below it pointed at an in-pool page of NaN: the
    outputs equal the clean run bit for bit, split or not."""
    d = 128
    for sq in (1, 16):
        _, (q, k, v), _ = _inputs(DB, HQ, HKV, sq, DCAP, d, dtype, False)
        k, v = k.to(FP8).to(dtype), v.to(FP8).to(dtype)
        lo = [max(0, n - sq + 1 - window) for n in DLENS]
        for ns in (1, 3, 0):
            # each form against its own clean run (the FP8 decode kernel sums a score's
            # products in another order than the 16-bit one: equal on exact sums only)
            for form, ps in [("contig", 0)] + DFORMS:
                clean = _decode_form(form, ps, q, k, v, DLENS, window, ns)
                got = _decode_form(form, ps, q, k, v, DLENS, window, ns, below=lo)
                assert dr.same(got, clean), (sq, ns, form, ps)


@pytest.mark.parametrize("paged", [False, True], ids=["contig", "paged"])
@pytest.mark.parametrize("dtype", dr.DTYPES)
def test_serving_loop_prefill_append_decode(dtype, paged):
    """Windowed prefill of a 200-token chunk behind 100 cached keys, one token
    appended, windowed decode of it: each step holds the references' gates on
    the cache as it then stands."""
    d, w, b, cap, pre, n = 128, 70, 2, 512, 100, 200
    _, (q, k, v), _ = _inputs(b, HQ, HKV, n, cap, d, dtype, False)
    q1 = _inputs(b, HQ, HKV, 1, cap, d, dtype, False)[1][0]
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
    got = pf(_lens(lens0), _lens(ql), return_lse=True, window=w)
    _check_f32(got, wr.refs(None, (q, *full()), lens0, ql, w, BF16), ql, dtype)
    gen = torch.Generator(device=DEV).manual_seed(9)
    kn = (torch.rand((b, HKV, 1, d), generator=gen, device=DEV) - 0.5).to(dtype)
    vn = (torch.rand((b, HKV, 1, d), generator=gen, device=DEV) - 0.5).to(dtype)
    ap(kn, vn, _lens(lens1))
    kf, vf = full()
    for bi in range(b):
        assert torch.equal(kf[bi, :, lens1[bi] - 1], kn[bi, :, 0])
    got = dc(_lens(lens1), return_lse=True, window=w)
    ref = wr.refs(None, (q1, kf, vf), lens1, None, w, BF16)
    _check_f32(got, ref, (1, 1), dtype)
    # the decode row equals a one-row windowed prefill of the same cache within the gates, too
    one = (prefill_paged(q1, kc, vc, table, _lens(lens1), None, return_lse=True, window=w) if paged
           else prefill(q1, kc, vc, _lens(lens1), None, return_lse=True, window=w))
    _check_f32(one, ref, (1, 1), dtype)


def _check_f32(got, refs, q_lens, dtype=F16):
    """The project's gates against the fp32-torch reference (for caches that
    exist on the device only): 1e-3 fp16 / 5e-3 bf16, LSE 2^-10 max|score| + 1e-5."""
    ro, lref, smax = refs
    gate = dr.GATE_F16 if dtype is F16 else dr.GATE_BF16
    for bi, n in enumerate(q_lens):
        if n:
            err = float((got[0][bi, :, :n].float() - ro[bi, :, :n]).abs().max())
            print(f"b={bi}: max_abs_diff {err:.3e}")
            assert err <= gate, (bi, err)
            dr.check_lse(got[1][bi:bi + 1, :, :n], lref[bi:bi + 1, :, :n], smax, f"b={bi}")
