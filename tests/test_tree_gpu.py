"""GPU tests of the tree-masked decode (include/fa_mi355x_tree.h) over the four
cache forms: the chain mask against the existing entries bit for bit, the
contract against tests/tree_refs.py's float64 reference at the decode gates,
census inputs where every visible key counts, the cache forms' bit identities,
the never-read range of a windowed paged call, graph capture and the torch ops.

Shapes (G, Sq) follow the row -> token map r % Sq and the NB choice: (1, 1);
(4, 4) NB 1; (5, 3) a ragged block; (3, 7) heads straddle a 16-row block and r %
Sq is unaligned; (4, 8) NB 2; (8, 8) NB 4, the register-tight kernel at D =
128; (8, 16) two row groups.  Lengths mix, in one call of B = 3: no keys, drafts
with negative rows (Sq - 2), no prefix (Sq), Sq + 1, a full tile, drafts that
straddle tiles 0 and 1 (two waves apply the mask), 65, drafts in different
pieces of a split (128 + Sq / 2 at num_splits 2 and 3) and 259."""
import numpy as np
import pytest
import torch

import decode_refs as dr
import fa_mi355x
import keysense_inputs as ks
import sink_refs as sr
import tree_refs as tr

pytestmark = pytest.mark.gpu

DEV = dr.DEV
FP8 = torch.float8_e4m3fn
F16, BF16 = torch.float16, torch.bfloat16
B, HKV, CAP = 3, 2, 320
SHAPES = [(1, 1), (4, 4), (5, 3), (3, 7), (4, 8), (8, 8), (8, 16)]
FORMS = ("", "_paged", "_kv8", "_paged_kv8")
SHAPE_IDS = ["g%dsq%d" % s for s in SHAPES]

decode = fa_mi355x.flash_attention_decode
decode_paged = fa_mi355x.flash_attention_decode_paged


def _len_sets(sq):
    return [(max(sq - 2, 0), sq, sq + 1), (0, 64, 64 + sq // 2), (65, 128 + sq // 2, 259)]


def _windows(sq):
    return (sq, 70, 200)


def _nan_rows(rows):
    if rows.element_size() == 1:
        rows.view(torch.uint8).fill_(0x7f)  # the E4M3 NaN
    else:
        rows.view(torch.int16).fill_(dr.NAN_BITS)


def _pad(t, lens, cap_to=None):
    """A copy with NaN bits in the rows at or past each length, the capacity
    grown to `cap_to` rows of the same."""
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


def _cache(form, k, v, lens, ps=64, seed=0, **scales):
    """run(q, **kw) -> (out, lse) over one cache form of the clean 16-bit k, v
    (a kv8 form reads their E4M3 conversion), NaN past every length."""
    if form.endswith("kv8"):
        k, v = k.to(FP8), v.to(FP8)
    tl = dr.lens(lens)
    if "paged" in form:
        kp, vp, table = _paginate(k, v, ps, lens, seed=seed + ps, filler="junk")
        return lambda q, **kw: decode_paged(q, kp, vp, table, tl, return_lse=True, **scales, **kw)
    kc, vc = _pad(k, lens), _pad(v, lens)
    return lambda q, **kw: decode(q, kc, vc, tl, return_lse=True, **scales, **kw)


def _qkv(g, sq, d, dtype, seed=42):
    """decode_refs.inputs as tensors of `dtype` (bf16: the fp16 values rounded)."""
    return tuple(dr.dev(a).to(dtype) for a in dr.inputs(B, g * HKV, HKV, sq, CAP, d, seed))


def _e4m3(t):
    """Values every cache form holds exactly."""
    return t.to(FP8).to(t.dtype)


class _NullMask:
    """tree_mask = NULL through the Python call path (the C entries' chain)."""

    @staticmethod
    def data_ptr():
        return None


def _null_mask_call(form, k, v, lens, ps=64, seed=0):
    """_cache's run() on the tree entry with a NULL mask."""
    kv8 = form.endswith("kv8")
    if kv8:
        k, v = k.to(FP8), v.to(FP8)
    tl = dr.lens(lens)
    table = None
    if "paged" in form:
        k, v, table = _paginate(k, v, ps, lens, seed=seed + ps, filler="junk")
    else:
        k, v = _pad(k, lens), _pad(v, lens)

    def run(q, window=0, sinks=None, num_splits=0):
        return fa_mi355x._decode_call(kv8, q, k, v, torch.empty_like(q), table, tl, True, True, num_splits, None,
                                      None, None, window, sinks, _NullMask())
    return run


# ---- 1. the chain, bit for bit ----------------------------------------------------------

@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("dtype", dr.DTYPES)
@pytest.mark.parametrize("g,sq", SHAPES, ids=SHAPE_IDS)
def test_chain_mask_equals_the_existing_entries(g, sq, dtype, d):
    """tree_mask = the chain (2 << t) - 1, and NULL at the C entry, give the
    plain, `_win` and `_sink` entries' O and LSE bit for bit at the same window,
    sinks and num_splits, in every cache form."""
    q, k, v = _qkv(g, sq, d, dtype)
    chain = tr.to_device(tr.masks("chain", B, sq))
    sinks = sr.draw_sinks(g * HKV, 7).to(DEV)
    w = _windows(sq)[(g + sq) % 3]
    for lens in _len_sets(sq):
        for form in FORMS:
            run = _cache(form, k, v, lens, ps=64 if sq % 2 else 128)
            null = _null_mask_call(form, k, v, lens, ps=64 if sq % 2 else 128)
            for kw in (dict(), dict(window=w), dict(sinks=sinks), dict(window=w, sinks=sinks)):
                for ns in (1, 2, 3):
                    want = run(q, num_splits=ns, **kw)
                    what = f"{lens} {form or 'contig'} {sorted(kw)} ns={ns}"
                    assert dr.same(run(q, num_splits=ns, tree_mask=chain, **kw), want), what
                    assert dr.same(null(q, num_splits=ns, **kw), want), "NULL " + what


# ---- 2. the contract against the float64 reference ---------------------------------------

def _mask_cases(sq):
    """(kind, window, with sinks): every kind with and without a window and sinks."""
    w = _windows(sq)
    return [("star", 0, False), ("star", w[1], True), ("binary", w[0], False), ("binary", w[2], True),
            ("random_tree", w[1], False), ("random_tree", 0, True), ("arbitrary", w[0], True),
            ("arbitrary", w[2], False)]


@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("dtype", dr.DTYPES)
@pytest.mark.parametrize("g,sq", SHAPES, ids=SHAPE_IDS)
def test_masks_against_the_float64_reference(g, sq, dtype, d):
    """Star, binary, random-tree and arbitrary masks, with and without a window
    and sinks, unsplit and split, contiguous and paged: O at the decode gates,
    the LSE at decode_refs.check_lse's."""
    q, k, v = _qkv(g, sq, d, dtype)
    gate = dr.GATE_F16 if dtype is F16 else dr.GATE_BF16
    sinks = sr.draw_sinks(g * HKV, 3)
    sinks[0] = float("-inf")
    for li, lens in enumerate(_len_sets(sq)[1:]):
        runs = [("contig", _cache("", k, v, lens)), ("paged", _cache("_paged", k, v, lens, ps=64 + 64 * li))]
        for ci, (kind, w, with_sinks) in enumerate(_mask_cases(sq)):
            words = tr.masks(kind, B, sq, seed=ci)
            seen = tr.vis(words, lens, sq, CAP, w)
            s = sinks if with_sinks else None
            ref = tr.contract_f64(q, k, v, seen, s)
            kw = dict(tree_mask=tr.to_device(words), window=w, sinks=None if s is None else s.to(DEV))
            for name, run in runs:
                for ns in (1, 2, 3) if li else (1, 2):
                    o, lse = run(q, num_splits=ns, **kw)
                    tr.check(o, lse, ref, seen, gate, f"{kind} W={w} sinks={with_sinks} {lens} {name} ns={ns}")


# ---- 3. every key counts ------------------------------------------------------------------

CENSUS_D64 = ((5, 3), (3, 7), (8, 16))  # one shape per NB also at D = 64; every shape at D = 128


@pytest.mark.parametrize("dtype", dr.DTYPES)
@pytest.mark.parametrize("g,sq", SHAPES, ids=SHAPE_IDS)
def test_census_of_the_visible_keys(g, sq, dtype):
    """Census inputs (every score equal, V zeros and ones): the number of visible
    keys read back from O and from the LSE is exact for every row, so a draft
    key lost, doubled or taken from another row's or element's word fails at any
    length; rows that see no key (a zero word and no prefix) are exact zeros.
    D = 128 at every shape, and D = 64 at one shape per NB (CENSUS_D64)."""
    for d in (128, 64) if (g, sq) in CENSUS_D64 else (128,):
        _census_of_the_visible_keys(g, sq, dtype, d)


def _census_of_the_visible_keys(g, sq, dtype, d):
    hq, level = g * HKV, 0.25
    score = level * level * d / np.sqrt(d)
    sinks, m = sr.census_sinks(hq, score)
    for layout in ks.census_layouts(CAP, d):
        q, k, v, _ = ks.census_qkv((B, hq, sq, d), (B, HKV, CAP, d), level, layout, dtype, DEV)
        v01 = ks.census_v(CAP, d, layout)
        for li, lens in enumerate(_len_sets(sq)):
            for fi, form in enumerate(FORMS):
                run = _cache(form, k, v, lens, ps=128 if fi % 2 else 64, seed=li)
                for ki, kind in enumerate(tr.KINDS):
                    w = (0, _windows(sq)[(ki + li) % 3])[(ki + fi) % 2]
                    words = tr.masks(kind, B, sq, seed=li + fi)
                    seen = tr.vis(words, lens, sq, CAP, w)
                    with_sinks = (ki + li + fi) % 2 == 1
                    ns = 1 + (ki + fi) % 3
                    o, lse = run(q, num_splits=ns, tree_mask=tr.to_device(words), window=w,
                                 sinks=sinks.to(DEV) if with_sinks else None)
                    gate = 2.0 ** -10 * max(abs(score), float(sinks.abs().max())) + 1e-5 if with_sinks else None
                    tr.check_census(o, lse, v01, seen, score,
                                    f"{layout} {lens} {form or 'contig'} {kind} W={w} sinks={with_sinks} ns={ns}",
                                    m=m if with_sinks else None, lse_gate=gate)
                    if kind == "arbitrary" and li == 0:
                        assert not seen[:, :, :].any(-1).all(), "no empty row in this case"


@pytest.mark.parametrize("form", FORMS)
def test_needle_in_a_draft_key_only_its_row_sees(form):
    """Star masks (the root plus self): draft key t >= 1 is visible to row t
    alone, and every row's query points at its own draft key, so each row must
    read exactly that key: with another row's or element's word it could not."""
    g, sq, d, dtype = 3, 7, 128, F16
    hq = g * HKV
    k, v = ks.needle_kv((B, HKV), CAP, d, 5, dtype, DEV)
    lens = (64 + sq // 2, 259, sq)
    words = np.stack([[1 | (1 << t) for t in range(sq)]] * B)
    pi = torch.tensor([[[ln - sq + t for t in range(sq)]] * hq for ln in lens])
    seen = tr.vis(words, lens, sq, CAP)
    assert all(seen[b, :, lens[b] - sq + t].sum() == 1 for b in range(B) for t in range(1, sq))
    q = ks.needle_q(k, pi, g)
    for ns in (1, 2):
        o, lse = _cache(form, k, v, lens)(q, num_splits=ns, tree_mask=tr.to_device(words))
        ref = torch.from_numpy(tr.contract_f64(q, k, v, seen)[1])
        ks.check_needle(o, ks.needle_expected(v, pi, g), pi, f"needle {form or 'contig'} ns={ns}", lse, ref,
                        d).require()


# ---- 4. bit identities of the cache forms ---------------------------------------------------

def _exact_inputs(kind, g, sq, d, dtype):
    """(q, k, v) whose score sums are exact in any order: census (one level, V
    zeros and ones) or needle (K of +-1, Q = 4 K[the row's own draft key of
    element 0's length])."""
    hq = g * HKV
    if kind == "census":
        return ks.census_qkv((B, hq, sq, d), (B, HKV, CAP, d), 0.25, "stripe", dtype, DEV)[:3]
    k, v = ks.needle_kv((B, HKV), CAP, d, 7, dtype, DEV)
    pi = torch.tensor([[[100 + t for t in range(sq)]] * hq] * B)
    return ks.needle_q(k, pi, g), k, v


@pytest.mark.parametrize("dtype", dr.DTYPES)
@pytest.mark.parametrize("g,sq", [(5, 3), (8, 8), (8, 16)], ids=["g5sq3", "g8sq8", "g8sq16"])
def test_cache_forms_are_bit_identical(g, sq, dtype):
    """Random-tree masks.  Paged equals contiguous on the gathered cache, 16-bit
    and FP8, on any input (random values, exact in E4M3).  An FP8 cache with
    unit scales equals the 16-bit one where the `_sink` twin does: the FP8
    decode kernel adds a score's products over d in another order (DESIGN.md
    section 3.0i, 3.0m), so the identity is the twin's on inputs whose score
    sums are exact, census and needle, and is asserted on those."""
    d = 128
    sinks = sr.draw_sinks(g * HKV, 2).to(DEV)
    one = torch.ones(HKV, device=DEV)
    q, k, v = _qkv(g, sq, d, dtype, seed=9)
    cases = [("random", q, _e4m3(k), _e4m3(v))] + [(kind, *_exact_inputs(kind, g, sq, d, dtype))
                                                     for kind in ("census", "needle")]
    for li, lens in enumerate(_len_sets(sq)):
        mask = tr.to_device(tr.masks("random_tree", B, sq, seed=li))
        for kw in (dict(), dict(window=_windows(sq)[li], sinks=sinks)):
            for ns in (1, 3):
                for kind, q, k, v in cases:
                    run = lambda form, ps=64, **sc: _cache(form, k, v, lens, ps=ps, **sc)(
                        q, num_splits=ns, tree_mask=mask, **kw)
                    what = (kind, lens, sorted(kw), ns)
                    want, want8 = run(""), run("_kv8")
                    for ps in (64, 128):
                        assert dr.same(run("_paged", ps), want), ("paged", ps) + what
                        assert dr.same(run("_paged_kv8", ps), want8), ("paged kv8", ps) + what
                    assert dr.same(run("_kv8", k_scale=one, v_scale=one), want8), ("unit scales",) + what
                    if kind != "random":
                        assert dr.same(want8, want), ("kv8 = 16-bit",) + what


# ---- 5. never read ----------------------------------------------------------------------------

@pytest.mark.parametrize("kv8", [False, True], ids=["16bit", "kv8"])
def test_rows_and_pages_below_the_window_are_never_read(kv8):
    """A windowed paged call: the table entries of pages wholly below len - Sq +
    1 - W hold out-of-pool ids and the cache rows below that key hold NaN; the
    result is finite and bit-equal to the clean call (the `_win` tests' form)."""
    g, sq, d, ps, w = 8, 8, 128, 64, 70
    q, k, v = _qkv(g, sq, d, F16, seed=4)
    lens = (259, 130, 64 + sq // 2)
    if kv8:
        k, v = k.to(FP8), v.to(FP8)
    mask = tr.to_device(tr.masks("random_tree", B, sq, seed=1))
    sinks = sr.draw_sinks(g * HKV, 1).to(DEV)
    kp, vp, table = _paginate(k, v, ps, lens, seed=3)
    first = tr.first_visible(lens, B, sq, CAP, w)
    assert first[0] // ps >= 2 and first[0] % ps and first[2] == 0
    dirty_t, dk, dv = table.clone(), kp.clone(), vp.clone()
    for bi, f in enumerate(first):
        for j in range(f // ps):
            dirty_t[bi, j] = kp.shape[0] + 7 + j  # wholly below: never looked up
        if f % ps:
            pg = int(table[bi, f // ps])
            _nan_rows(dk[pg, :, :f % ps])
            _nan_rows(dv[pg, :, :f % ps])
    tl = dr.lens(lens)
    for ns in (1, 2):
        kw = dict(return_lse=True, num_splits=ns, window=w, sinks=sinks, tree_mask=mask)
        clean = decode_paged(q, kp, vp, table, tl, **kw)
        dirty = decode_paged(q, dk, dv, dirty_t, tl, **kw)
        assert bool(torch.isfinite(dirty[0]).all()) and bool(torch.isfinite(dirty[1]).all())
        assert dr.same(dirty, clean), ns


# ---- 6. graph capture ---------------------------------------------------------------------------

def test_a_captured_graph_follows_the_mask_the_lengths_and_the_sinks():
    g, sq, d, w = 8, 8, 128, 70
    q, k, v = _qkv(g, sq, d, F16, seed=6)
    cases = [("random_tree", (259, 130, 64 + sq // 2), 11), ("arbitrary", (sq, 200, 65), 12),
             ("star", (0, 320, 131), 13)]
    mask = tr.to_device(tr.masks(cases[0][0], B, sq))
    tl = dr.lens(cases[0][1])
    ts = sr.draw_sinks(g * HKV, cases[0][2]).to(DEV)
    out = torch.empty_like(q)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        call = lambda: decode(q, k, v, tl, out=out, return_lse=True, num_splits=3, window=w, sinks=ts,
                              tree_mask=mask)
        call()  # warm-up outside the capture
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            res = call()
    torch.cuda.current_stream().wait_stream(stream)
    for kind, lens, seed in cases[1:] + cases[:1]:
        words = tr.masks(kind, B, sq, seed)
        s = sr.draw_sinks(g * HKV, seed)
        mask.copy_(tr.to_device(words))
        tl.copy_(dr.lens(lens))
        ts.copy_(s.to(DEV))
        graph.replay()
        torch.cuda.synchronize()
        want = decode(q, k, v, dr.lens(lens), return_lse=True, num_splits=3, window=w, sinks=s.to(DEV),
                      tree_mask=tr.to_device(words))
        assert dr.same(res, want), (kind, lens)
        assert dr.ws_counters_zero()
        seen = tr.vis(words, lens, sq, CAP, w)
        tr.check(*res, tr.contract_f64(q, k, v, seen, s), seen, dr.GATE_F16, f"graph {kind} {lens}")


# ---- 7. torch ops ---------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", dr.DTYPES)
def test_torch_ops_equal_the_python_functions(dtype):
    import fa_mi355x.torch_op_tree  # noqa: F401 (registers the ops)

    g, sq, d = 4, 8, 128
    q, k, v = _qkv(g, sq, d, dtype, seed=8)
    lens = (259, 64 + sq // 2, sq)
    tl = dr.lens(lens)
    mask = tr.to_device(tr.masks("random_tree", B, sq, seed=2))
    sinks = sr.draw_sinks(g * HKV, 4).to(DEV)
    ksc, vsc = torch.tensor([0.5, 2.0], device=DEV), torch.tensor([0.25, 1.5], device=DEV)
    op, op_paged = torch.ops.fa_mi355x_tree.decode, torch.ops.fa_mi355x_tree.decode_paged
    for kv8 in (False, True):
        kc, vc = (_pad(x.to(FP8) if kv8 else x, lens) for x in (k, v))
        kp, vp, table = _paginate(kc, vc, 64, lens, seed=5)
        sc = dict(k_scale=ksc, v_scale=vsc) if kv8 else {}
        for kw in (dict(), dict(window=70), dict(sinks=sinks), dict(window=sq, sinks=sinks)):
            want = decode(q, kc, vc, tl, tree_mask=mask, **sc, **kw)
            assert torch.equal(op(q, kc, vc, mask, tl, **sc, **kw), want), (kv8, sorted(kw))
            want = decode_paged(q, kp, vp, table, tl, tree_mask=mask, **sc, **kw)
            assert torch.equal(op_paged(q, kp, vp, table, mask, tl, **sc, **kw), want), (kv8, sorted(kw))
    # positional, a strided q (made contiguous) and a strided cache (refused, never copied)
    qs = q.transpose(1, 2).contiguous().transpose(1, 2)
    assert torch.equal(op(qs, kc, vc, mask, tl, ksc, vsc, 70, sinks),
                       decode(q, kc, vc, tl, k_scale=ksc, v_scale=vsc, window=70, sinks=sinks, tree_mask=mask))
    with pytest.raises(fa_mi355x.FlashAttentionError, match="k_cache must be contiguous"):
        op(q, kc[:, :, ::2], vc[:, :, ::2], mask, tl)


# ---- 8. the wrappers' rules on device tensors ------------------------------------------------------

def test_wrapper_rules_on_device_tensors():
    fa = fa_mi355x
    g, sq, d = 4, 4, 64
    q, k, v = _qkv(g, sq, d, F16)
    mask = tr.to_device(tr.masks("binary", B, sq))
    for bad, status, msg in ((mask.cpu(), fa.FA_ERR_NULL_POINTER, "tree_mask must be a tensor on cuda"),
                             (mask.long(), fa.FA_ERR_BAD_SHAPE, "tree_mask must be a contiguous int32")):
        with pytest.raises(fa.FlashAttentionError, match=msg) as e:
            decode(q, k, v, tree_mask=bad)
        assert e.value.status == status
    with pytest.raises(fa.FlashAttentionError, match="tree_mask needs causal=True") as e:
        decode(q, k, v, tree_mask=mask, causal=False)
    assert e.value.status == fa.FA_ERR_BAD_SHAPE
    with pytest.raises(fa.FlashAttentionError, match="a window must be 0 or >= Sq = 4") as e:
        decode(q, k, v, tree_mask=mask, window=3)
    assert e.value.status == fa.FA_ERR_BAD_SHAPE
    # kv_lens = None: every length is the capacity
    seen = tr.vis(tr.masks("binary", B, sq), None, sq, CAP, 4)
    o, lse = decode(q, k, v, tree_mask=mask, window=4, return_lse=True)
    tr.check(o, lse, tr.contract_f64(q, k, v, seen), seen, dr.GATE_F16, "kv_lens=None")
