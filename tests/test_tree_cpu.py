"""CPU tests of the tree-masked decode (no GPU): fa_mi355x.TREE_ENTRIES against
the declarations of include/fa_mi355x_tree.h, the C entries' statuses with fake
pointers, the Python wrappers' argument errors, tree_mask_from_parents against
a loop, the references of tests/tree_refs.py against the chain's existing ones,
the new units' kernel resources and the torch ops under FakeTensorMode."""
import ctypes
import re
import types

import numpy as np
import pytest
import torch

import capi_checks as cc
import decode_refs as dr
import fa_mi355x
import keysense_inputs as ks
import sink_refs as sr
import tree_refs as tr
import window_refs as wr

err = fa_mi355x.FlashAttentionError
FORMS = ("", "_paged", "_kv8", "_paged_kv8")
UNITS = ["fa_decode_tree%s.hip" % f for f in FORMS]


# ---- header and table ---------------------------------------------------------------

SCALARS = {"int": ctypes.c_int, "unsigned long long": ctypes.c_ulonglong}
POINTERS = {"const void*", "void*", "const int*", "const float*", "float*"}


def _ctype(decl):
    ty = re.sub(r"\b[A-Za-z_]\w*$", "", decl)  # the parameter's name
    ty = re.sub(r"\s*\*\s*", "*", " ".join(ty.split()))
    if ty in SCALARS:
        return SCALARS[ty]
    assert ty in POINTERS, f"a type this test has no mapping for: {ty!r} in {decl!r}"
    return ctypes.c_void_p


def _declarations():
    """[(name, restype, argtypes, parameter names)] of every function
    fa_mi355x_tree.h declares (test_binding_table_cpu.py's regex)."""
    found = re.findall(r"^([A-Za-z_][\w \*]*?)\b([a-z_][a-z0-9_]*)\s*\(([^;{]*)\)\s*;",
                       cc.header_text("fa_mi355x_tree.h"), re.M)
    out = []
    for ret, name, params in found:
        params = [p.strip() for p in params.split(",")]
        assert ret.strip() == "int", (name, ret)
        out.append((name, ctypes.c_int, [_ctype(p) for p in params], [p.split()[-1].lstrip("*") for p in params]))
    return out


def test_table_matches_the_header():
    decls = _declarations()
    names = [d[0] for d in decls]
    assert len(names) == len(set(names)) == 8
    assert set(names) == set(fa_mi355x.TREE_ENTRIES) == {
        "fa_decode_tree%s_%s" % (f, ty) for f in FORMS for ty in ("f16", "bf16")}
    wrong = [(n, a, fa_mi355x.TREE_ENTRIES[n]) for n, r, a, _ in decls if fa_mi355x.TREE_ENTRIES[n] != (r, a)]
    assert not wrong, wrong[:2]
    # the `_sink` twin's list with tree_mask directly after sinks
    sink = dict((n, p) for n, p in re.findall(r"\b(fa_decode_sink\w+)\s*\(([^;{]*)\)\s*;", cc.header_text("fa_mi355x.h")))
    for name, _, argtypes, params in decls:
        twin = [p.split()[-1].lstrip("*") for p in sink[name.replace("_tree", "_sink")].split(",")]
        at = twin.index("sinks") + 1
        assert params == twin[:at] + ["tree_mask"] + twin[at:], name
        assert fa_mi355x.C_ENTRIES[name.replace("_tree", "_sink")][1] == argtypes[:at] + argtypes[at + 1:], name
    lists = [id(a) for _, a in fa_mi355x.TREE_ENTRIES.values()]
    assert len(lists) == len(set(lists))


def test_the_two_tables_stay_apart():
    assert not set(fa_mi355x.C_ENTRIES) & set(fa_mi355x.TREE_ENTRIES)
    assert len(fa_mi355x.C_ENTRIES) == 132 and fa_mi355x.EXPORTED_SYMBOLS == tuple(fa_mi355x.C_ENTRIES)
    assert "fa_mi355x_tree.h" not in cc.header_text("fa_mi355x.h")
    assert '#include "fa_mi355x.h"' in cc.header_text("fa_mi355x_tree.h")


def test_exported_and_typed():
    syms = cc.exported_symbols()
    lib = fa_mi355x.load_library()
    for name, (restype, argtypes) in fa_mi355x.TREE_ENTRIES.items():
        assert name in syms, name
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
    assert fa_mi355x._entry_name("fa_decode", "_tree", True, True, True) == "fa_decode_tree_paged_kv8_bf16"


# ---- statuses through the C entries (fake pointers: all returned before any launch) ---

P = ctypes.c_void_p(0x1000)


def _call(form, ty="_f16", q=P, k=P, v=P, o=P, b=1, hq=8, hkv=2, sq=4, cap=1024, d=128, psz=128, table=P,
          lens=None, causal=1, window=0, sinks=None, mask=P, ns=0, ws=None, wsb=0):
    fn = getattr(fa_mi355x.load_library(), "fa_decode_tree" + form + ty)
    cache = [d, 100, psz, table, cap // 128] if "paged" in form else [cap, d]
    scales = [None, None] if "kv8" in form else []
    return fn(q, k, v, o, None, b, hq, hkv, sq, *cache, lens, causal, window, sinks, mask, ns, ws, wsb, None,
              *scales)


@pytest.mark.parametrize("ty", ["_f16", "_bf16"])
@pytest.mark.parametrize("form", FORMS)
def test_tree_statuses(form, ty):
    fa = fa_mi355x
    call = lambda **kw: _call(form, ty, **kw)
    # the mask replaces the causal rule
    assert call(causal=0) == fa.FA_ERR_BAD_SHAPE
    assert call(causal=0, mask=None) == fa.FA_ERR_BAD_SHAPE
    # a window shorter than the drafts; Sq itself and longer ones are shapes (the
    # plan of this one wants a workspace, the next status in line)
    for w in (1, 2, 3):
        assert call(window=w) == fa.FA_ERR_BAD_SHAPE, w
    for w in (0, 4, 5, 70, 1 << 30):
        assert call(window=w, ns=2) == fa.FA_ERR_WORKSPACE, w
    assert call(window=1, sq=1, ns=2) == fa.FA_ERR_WORKSPACE
    assert call(window=-1) == fa.FA_ERR_BAD_SHAPE
    # the twin's order: negative shapes and window, head_dim, seqlen_q, then causal / window
    assert call(causal=0, d=96) == fa.FA_ERR_UNSUPPORTED_HEAD_DIM
    assert call(window=2, d=96) == fa.FA_ERR_UNSUPPORTED_HEAD_DIM
    assert call(window=-1, d=96) == fa.FA_ERR_BAD_SHAPE
    assert call(causal=0, sq=17) == fa.FA_ERR_BAD_SHAPE
    # ... and before the pointers, the heads and the workspace
    assert call(causal=0, q=None) == fa.FA_ERR_BAD_SHAPE
    assert call(window=2, q=None, hq=7) == fa.FA_ERR_BAD_SHAPE
    assert call(q=None) == fa.FA_ERR_NULL_POINTER
    # an empty batch: nothing to do, but the two rules are shapes and still hold
    assert call(b=0, q=None, k=None, v=None, o=None, mask=None) == fa.FA_OK
    assert call(b=0, causal=0) == fa.FA_ERR_BAD_SHAPE
    # a NULL mask is the chain, not an error: the next status is the workspace's
    assert call(mask=None, ns=2) == fa.FA_ERR_WORKSPACE
    if "paged" in form:
        assert call(psz=32) == fa.FA_ERR_BAD_SHAPE
        assert call(table=None) == fa.FA_ERR_NULL_POINTER


def _shim(paged, kv8, window, sinks, mask):
    """The loaded library with fa_decode[_paged]_f16 / _bf16 bound to the tree
    entries at a fixed window, sinks and mask pointer, for capi_checks' decode
    tables (test_sinks_cpu.py's shim, one argument more)."""
    lib = fa_mi355x.load_library()
    shim = types.SimpleNamespace(fa_decode_ws_bytes=lib.fa_decode_ws_bytes,
                                 fa_decode_num_splits=lib.fa_decode_num_splits)
    at = 15 if paged else 12  # the arguments up to and including causal

    def bind(fn):
        tail = (None, None) if kv8 else ()
        return lambda *a: fn(*a[:at + 1], window, sinks, mask, *a[at + 1:], *tail)

    form = ("_paged" if paged else "") + ("_kv8" if kv8 else "")
    for ty in ("_f16", "_bf16"):
        setattr(shim, "fa_decode" + ("_paged" if paged else "") + ty,
                bind(getattr(lib, "fa_decode_tree" + form + ty)))
    return shim


@pytest.mark.parametrize("kv8", [False, True], ids=["16bit", "kv8"])
@pytest.mark.parametrize("paged", [False, True], ids=["contig", "paged"])
def test_decode_twins_tables_with_a_mask(paged, kv8):
    """capi_checks' whole decode tables (workspace statuses included) hold for
    the tree entries as they do for the `_sink` twins, at the twins' test's
    windows, with and without sinks and a mask."""
    for w in (4096, 0):
        for sinks in (None, P):
            for mask in (None, P):
                shim = _shim(paged, kv8, w, sinks, mask)
                (cc.decode_paged_argument_checks if paged else cc.decode_argument_checks)(fa_mi355x, shim)


# ---- the Python wrappers ---------------------------------------------------------------

def _t(shape, dtype=torch.float16):
    return torch.zeros(shape, dtype=torch.float32).to(dtype)


def _wrapper_calls():
    fa = fa_mi355x
    qd, k = _t((2, 4, 3, 64)), _t((2, 2, 128, 64))
    table = torch.zeros((2, 2), dtype=torch.int32)
    return [lambda **kw: fa.flash_attention_decode(qd, k, k, **kw),
            lambda **kw: fa.flash_attention_decode_paged(qd, k, k, table, **kw)]


def test_wrapper_rejections():
    """tree_mask is checked in sinks' wording and place: int32, [B, Sq],
    contiguous, a tensor -> FA_ERR_BAD_SHAPE before where the tensors live; its
    values are not looked at; then its device, causal and the window."""
    fa = fa_mi355x
    good = torch.zeros((2, 3), dtype=torch.int32)
    bad = [
        (torch.zeros((2, 3), dtype=torch.int64), r"got torch.int64 \[2, 3\]"),
        (torch.zeros((2, 3), dtype=torch.uint8), r"got torch.uint8 \[2, 3\]"),
        (torch.zeros((2, 3), dtype=torch.float32), r"got torch.float32 \[2, 3\]"),
        (torch.zeros((2, 3), dtype=torch.bool), r"got torch.bool \[2, 3\]"),
        (torch.zeros((3, 2), dtype=torch.int32), r"got torch.int32 \[3, 2\]"),
        (torch.zeros((2, 4), dtype=torch.int32), r"got torch.int32 \[2, 4\]"),
        (torch.zeros((1, 3), dtype=torch.int32), r"got torch.int32 \[1, 3\]"),
        (torch.zeros((6,), dtype=torch.int32), r"got torch.int32 \[6\]"),
        (torch.zeros((2, 4, 3), dtype=torch.int32), r"got torch.int32 \[2, 4, 3\]"),
        (torch.zeros((2, 6), dtype=torch.int32)[:, ::2], r"got torch.int32 \[2, 3\]"),  # not contiguous
        (torch.zeros((3, 2), dtype=torch.int32).t(), r"got torch.int32 \[2, 3\]"),
        ([[0] * 3] * 2, "got list"),
    ]
    for f in _wrapper_calls():
        for m, got in bad:
            for kw in (dict(), dict(window=8, sinks=torch.zeros(4))):
                with pytest.raises(err, match=r"tree_mask must be a contiguous int32 \[B = 2, Sq = 3\] tensor, "
                                   + got) as e:
                    f(tree_mask=m, **kw)
                assert e.value.status == fa.FA_ERR_BAD_SHAPE
        # a bad window is named first, then sinks, whatever the mask is
        with pytest.raises(err, match=r"window must be >= 0"):
            f(tree_mask=bad[0][0], window=-1)
        with pytest.raises(err, match="sinks must be a contiguous float32"):
            f(tree_mask=bad[0][0], sinks=torch.zeros(5))
        # a good mask (any values): what is left is where the tensors live, as without one
        for m in (good, torch.full((2, 3), -1, dtype=torch.int32)):
            with pytest.raises(err, match="q must be a device tensor") as e:
                f(tree_mask=m)
            assert e.value.status == fa.FA_ERR_NULL_POINTER
        with pytest.raises(err, match="q must be a device tensor"):
            f()
    # the device stage and the two rules, which the wrappers reach on device tensors only
    q = _t((2, 4, 3, 64))
    with pytest.raises(err, match="tree_mask must be a tensor on cpu") as e:
        fa._check_tree_mask(q, good, True)
    assert e.value.status == fa.FA_ERR_NULL_POINTER
    fa._check_tree_mask(q, good, False)
    fa._check_tree_mask(q, None, True)
    with pytest.raises(err, match="tree_mask needs causal=True") as e:
        fa._check_tree_rules(q, False, 0)
    assert e.value.status == fa.FA_ERR_BAD_SHAPE
    for w in (1, 2):
        with pytest.raises(err, match=r"a window must be 0 or >= Sq = 3 .*got %d" % w) as e:
            fa._check_tree_rules(q, True, w)
        assert e.value.status == fa.FA_ERR_BAD_SHAPE
    for w in (0, 3, 4, 1 << 31):
        fa._check_tree_rules(q, True, w)


# ---- tree_mask_from_parents -------------------------------------------------------------

@pytest.mark.parametrize("sq", [1, 2, 3, 7, 8, 9, 16])
def test_tree_mask_from_parents(sq):
    for gen in (tr.chain_parents, tr.star_parents, tr.binary_parents, tr.random_parents):
        for seed in range(3):
            parents = gen(5, sq, seed)
            want = tr.masks_from_parents(parents)
            for dtype in (torch.int32, torch.int64, torch.int16):
                got = fa_mi355x.tree_mask_from_parents(torch.from_numpy(parents).to(dtype))
                assert got.dtype == torch.int32 and got.shape == (5, sq) and got.is_contiguous()
                assert np.array_equal(got.numpy().astype(np.int64), want), (gen.__name__, seed)
    chain = fa_mi355x.tree_mask_from_parents(torch.from_numpy(tr.chain_parents(2, sq)))
    assert chain[0].tolist() == [(2 << t) - 1 for t in range(sq)]


def test_tree_mask_from_parents_rejections():
    for bad in (torch.zeros((2, 17), dtype=torch.int32), torch.zeros((2, 0), dtype=torch.int32),
                torch.zeros((4,), dtype=torch.int32), torch.zeros((2, 4)), torch.zeros((2, 4), dtype=torch.bool),
                [[-1, 0]]):
        with pytest.raises(err, match="parents must be an integer") as e:
            fa_mi355x.tree_mask_from_parents(bad)
        assert e.value.status == fa_mi355x.FA_ERR_BAD_SHAPE


# ---- reference sanity ---------------------------------------------------------------------

LENS = {1: (0, 1, 65), 3: (1, 3, 66), 4: (2, 5, 130), 7: (0, 7, 67), 16: (14, 17, 200)}


@pytest.mark.parametrize("sq", sorted(LENS))
def test_chain_vis_is_the_causal_rule(sq):
    cap, lens = 256, LENS[sq]
    words = tr.masks("chain", len(lens), sq)
    assert words[0].tolist() == [(2 << t) - 1 for t in range(sq)]
    key = np.arange(cap)
    count = ks.decode_visible(lens, 1, sq, True)[:, 0, :]  # [B, Sq]
    assert np.array_equal(tr.vis(words, lens, sq, cap), key[None, None, :] < count[..., None])
    for w in (sq, sq + 1, 70, 200, 1 << 20):
        lo, hi = wr.interval(lens, None, len(lens), sq, cap, w)
        want = (key[None, None, :] >= lo[..., None]) & (key[None, None, :] < hi[..., None])
        assert np.array_equal(tr.vis(words, lens, sq, cap, w), want), w
        # no row of any mask sees a key below the `_win` twin's first key
        first = tr.first_visible(lens, len(lens), sq, cap, w)
        for kind in tr.KINDS:
            seen = tr.vis(tr.masks(kind, len(lens), sq, 3), lens, sq, cap, w)
            for bi, f in enumerate(first):
                assert not seen[bi, :, :f].any(), (kind, w, bi)


def test_masks_are_what_they_say():
    for sq in (1, 3, 8, 16):
        star = tr.masks("star", 3, sq)
        assert star[0].tolist() == [1 | (1 << t) for t in range(sq)]  # root plus self
        assert not np.array_equal(star[0], star[1]) or sq == 1
        arb = tr.masks("arbitrary", 4, sq)
        low = (1 << sq) - 1
        assert (arb & ~low).any() and ((arb & low) == 0).any(1).all() and (arb == 0).any()
        for kind in ("binary", "random_tree"):
            m = tr.masks(kind, 3, sq, 1)
            assert all((int(m[b, t]) >> t) & 1 and int(m[b, t]) < (2 << t) for b in range(3) for t in range(sq))
    with pytest.raises(AssertionError):
        tr.vis(tr.masks("chain", 1, 4), [8], 4, 64, 3)


def test_chain_reference_is_the_sink_contract():
    b, hq, hkv, sq, cap, d = 3, 4, 2, 4, 192, 64
    qh, kh, vh = dr.inputs(b, hq, hkv, sq, cap, d)
    q, k, v = (tr.f64(a) for a in (qh, kh, vh))
    lens = (2, 70, 133)
    sinks = sr.draw_sinks(hq)
    sinks[1] = float("-inf")
    words = tr.masks("chain", b, sq)
    for w in (0, 4, 70):
        for s in (None, sinks):
            o, lse, smax = tr.contract_f64(q, k, v, tr.vis(words, lens, sq, cap, w), s)
            ro, rl, _, rs = sr.contract_f64(q, k, v, lens, None, w, s, with_smax=True)
            assert np.abs(o - ro).max() <= 1e-14 and smax == pytest.approx(rs)
            assert np.array_equal(np.isneginf(lse), np.isneginf(rl))
            fin = np.isfinite(rl)
            assert np.abs(lse[fin] - rl[fin]).max() <= 1e-13


def test_census_expectation_on_the_chain():
    """tree_refs' census over a set of keys is keysense_inputs' over a prefix."""
    sq, cap, d, lens = 4, 192, 64, (3, 64, 130)
    for layout in ks.census_layouts(cap, d):
        v01 = ks.census_v(cap, d, layout)
        counts = ks.census_counts(v01)
        seen = tr.vis(tr.masks("chain", len(lens), sq), lens, sq, cap)
        o, lse, n = tr.census_expected(v01, seen, 0.0)
        want_n = torch.from_numpy(ks.decode_visible(lens, 1, sq, True))
        wo, wl = ks.census_expected(counts, want_n, 0.0)
        assert torch.equal(n[:, None], want_n) and torch.equal(o, wo) and torch.equal(lse, wl)


# ---- kernel resources ----------------------------------------------------------------------

def test_kernel_resource_usage():
    """The siblings' budget holds for every Treed<> instantiation: no scratch and
    no static LDS (decode's LDS is dynamic, as its siblings': the `_sink` units
    compiled alongside say the same).  Each unit holds its 12 Treed<> decode
    kernels beside the one-line LSE fill of an empty cache."""
    twins = ["fa_decode_sink%s.hip" % f for f in FORMS]
    usage = cc.kernel_resource_usage(UNITS + twins)
    for unit, twin, kernels, theirs in zip(UNITS, twins, usage[:4], usage[4:]):
        mine = [x for x in kernels if "fa_decode_kernel" in x[0]]
        other = [x for x in kernels if "fa_decode_kernel" not in x[0]]
        assert len(other) == 1 and "fa_sink_fill_lse_kernel" in other[0][0] and other[0][1:] == (0, 0), unit
        assert len(mine) == 12 and all("Treed" in x[0] and "Sinked" in x[0] and "Windowed" in x[0] for x in mine), unit
        assert all(scratch == 0 for _, scratch, _ in mine), (unit, [x for x in mine if x[1]])
        sib = [x for x in theirs if "fa_decode_kernel" in x[0]]
        assert len(sib) == 12 and not any("Treed" in x[0] for x in sib), twin
        assert [lds for _, _, lds in mine] == [lds for _, _, lds in sib], unit


# ---- torch ops -----------------------------------------------------------------------------

def test_tree_ops_under_fake_tensors():
    import fa_mi355x.torch_op as top
    import fa_mi355x.torch_op_tree as tot
    from torch._subclasses.fake_tensor import FakeTensorMode

    tail = ("Tensor tree_mask, Tensor? kv_lens=None, Tensor? k_scale=None, Tensor? v_scale=None, int window=0, "
            "Tensor? sinks=None) -> Tensor")
    assert str(tot.decode.default._schema) == \
        "fa_mi355x_tree::decode(Tensor q, Tensor k_cache, Tensor v_cache, " + tail
    assert str(tot.decode_paged.default._schema) == \
        "fa_mi355x_tree::decode_paged(Tensor q, Tensor k_pages, Tensor v_pages, Tensor block_table, " + tail
    assert tot.decode.overloads() == ["default"] and tot.decode_paged.overloads() == ["default"]
    # the other namespace keeps its packets: nothing of this one is in it
    assert top.decode.overloads() == ["default", "window", "sinks"]
    assert not hasattr(torch.ops.fa_mi355x, "decode_tree")
    with FakeTensorMode():
        for dtype in (torch.float16, torch.bfloat16):
            q = torch.empty((2, 8, 4, 128), dtype=dtype, device="cuda").transpose(1, 2).transpose(1, 2)
            qs = torch.empty((2, 4, 8, 128), dtype=dtype, device="cuda").transpose(1, 2)  # strided
            k = torch.empty((2, 2, 256, 128), dtype=dtype, device="cuda")
            k8 = torch.empty((2, 2, 256, 128), dtype=torch.float8_e4m3fn, device="cuda")
            pool = torch.empty((9, 2, 128, 128), dtype=dtype, device="cuda")
            table = torch.empty((2, 2), dtype=torch.int32, device="cuda")
            mask = torch.empty((2, 4), dtype=torch.int32, device="cuda")
            lens = torch.empty((2,), dtype=torch.int32, device="cuda")
            sc = torch.empty((2,), dtype=torch.float32, device="cuda")
            sinks = torch.empty((8,), dtype=torch.float32, device="cuda")
            for x in (q, qs):
                for o in (tot.decode(x, k, k, mask), tot.decode(x, k, k, mask, lens, window=70, sinks=sinks),
                          tot.decode(x, k8, k8, mask, lens, sc, sc, 4, sinks),
                          tot.decode_paged(x, pool, pool, table, mask, lens, window=4),
                          tot.decode_paged(x, pool, pool, table, mask, sinks=sinks)):
                    assert o.shape == (2, 8, 4, 128) and o.dtype == dtype and o.is_contiguous()
                    assert o.device.type == "cuda"
            with pytest.raises(Exception, match="tree_mask"):
                tot.decode(q, k, k, mask.view(-1))
            with pytest.raises(Exception, match="window >= 0"):
                tot.decode(q, k, k, mask, window=-1)
            with pytest.raises(RuntimeError, match="forward-only"):
                tot.decode(q.clone().requires_grad_(), k, k, mask)
    # CPU tensors: the same refusal as the other namespace's ops
    q, k = _t((2, 8, 4, 128)), _t((2, 2, 256, 128))
    mask = torch.zeros((2, 4), dtype=torch.int32)
    with pytest.raises(ValueError, match=r"fa_mi355x_tree::decode needs GPU tensors \(no CPU path\)"):
        tot.decode(q, k, k, mask)
    with pytest.raises(ValueError, match=r"fa_mi355x_tree::decode_paged needs GPU tensors \(no CPU path\)"):
        tot.decode_paged(q, _t((9, 2, 128, 128)), _t((9, 2, 128, 128)), torch.zeros((2, 2), dtype=torch.int32), mask)
    with pytest.raises(ValueError, match=r"fa_mi355x::decode needs GPU tensors \(no CPU path\)"):
        top.decode(q, k, k)


def test_the_census_check_sees_one_wrong_draft_key():
    """The checker's own sensitivity, on the CPU: the exact census of a mask
    passes, and fails once a row's set loses a draft key, gains one, or is
    another row's or another element's."""
    sq, cap, d, lens = 4, 192, 64, (4, 70, 131)
    v01 = ks.census_v(cap, d, "stripe")
    words = tr.masks("random_tree", len(lens), sq, 1)
    seen = tr.vis(words, lens, sq, cap)
    for dtype in (torch.float16, torch.bfloat16):
        o, lse, _ = tr.census_expected(v01, seen, 1.0)
        o, lse = o.expand(-1, 2, -1, -1).to(dtype), lse.expand(-1, 2, -1).float()
        tr.check_census(o, lse, v01, seen, 1.0, "exact")
        for bi, ln in enumerate(lens):
            t = sq - 1
            wrong = []
            lost = seen.copy()
            lost[bi, t, ln - 1] = False                       # its own key
            gained = seen.copy()
            free = [i for i in range(sq) if not seen[bi, t, ln - sq + i]]
            if free:
                gained[bi, t, ln - sq + free[0]] = True
                wrong.append(gained)
            other_row = seen.copy()
            other_row[bi, t] = seen[bi, t - 1]
            wrong += [lost, other_row]
            for bad in wrong:
                with pytest.raises(AssertionError):
                    tr.check_census(o, lse, v01, bad, 1.0, "one wrong key")
