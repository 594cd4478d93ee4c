"""CPU tests of tests/instantiation_matrix.py (no GPU): that its cells are
exactly the launch entries of the three forward families, that its four decode
geometries reach NB 1, 2, 4 and 1, that the closed forms the GPU test will hold
the kernels to are the float64 contracts' results on the matrix's own inputs,
and that each fault of instantiation_matrix.FAULTS, applied to a float64 model
and rounded to the output type, fails the gates in every cell it applies to (the
pattern of tests/test_keysense_cpu.py).  The first two need no built library."""
import functools

import numpy as np
import pytest
import torch

import decode_refs as dr
import fa_mi355x as fa
import instantiation_matrix as im
import prefill_refs as pr
import sink_refs as sr
import tree_refs as tr
import window_refs as wr

# what the three prefixes also match and the matrix leaves out, each with its reason
EXCLUDED = {
    "fa_decode_ws_bytes": "a sizing helper: launches nothing",
    "fa_decode_num_splits": "a planning helper: launches nothing",
    "fa_attn_varlen_bwd_f16": "the backward pass: a sweep of its own",
    "fa_attn_varlen_bwd_bf16": "the backward pass: a sweep of its own",
}
FAMILIES = ("fa_decode", "fa_prefill", "fa_attn_varlen")


def test_the_cells_are_exactly_the_forward_launch_entries():
    table = set(fa.C_ENTRIES) | set(fa.TREE_ENTRIES)
    assert set(EXCLUDED) <= table, sorted(set(EXCLUDED) - table)
    launch = {n for n in table if n.startswith(FAMILIES)} - set(EXCLUDED)
    cells = im.cells()
    assert len(cells) == len(set(cells)) == 300
    assert (len(im.decode_cells()), len(im.prefill_cells()), len(im.attn_cells())) == (192, 96, 12)
    named = {im.entry(c) for c in cells}
    assert named == launch, (sorted(launch - named), sorted(named - launch))
    assert len(named) == 24 + 8 + 48 + 6
    # the binding's own composition of the same names, where it has one
    for c in cells:
        if c.variant != "_tree":
            assert fa._entry_name(c.family, c.variant, "paged" in c.form, "kv8" in c.form, c.ty == "bf16") == im.entry(c)
        else:
            assert im.entry(c) in fa.TREE_ENTRIES


def _decode_geom_nb(heads_q, heads_kv, seqlen_q):
    """decode_geom's rule (csrc/fa_decode_host.hpp), restated."""
    rows = (heads_q // heads_kv) * seqlen_q
    return 1 if rows <= 16 else 2 if rows <= 32 else 4


def test_the_geometries_reach_every_nb():
    pairs = [im.DEC_GEOM[1], im.DEC_GEOM[2], im.DEC_GEOM[4], im.DEC_SERVING]
    assert pairs == [(5, 3), (7, 3), (16, 5), (5, 1)]
    assert [dr.nb(g, sq) for g, sq in pairs] == [1, 2, 4, 1]
    assert [_decode_geom_nb(g * im.DEC_HKV, im.DEC_HKV, sq) for g, sq in pairs] == [1, 2, 4, 1]
    for nb in im.NBS:
        for variant in im.DECODE_VARIANTS:
            assert all(dr.nb(g, sq) == nb for g, sq in im.decode_geoms(variant, nb))
    g, sq = im.DEC_GEOM[2]
    assert 16 % sq != 0 and g * sq > 16          # a head change inside the first 16-row block
    g, sq = im.DEC_GEOM[4]
    assert 64 < g * sq < 128                     # a second row group, partial
    # the window's lower edge lies mid-tile in both windowed lengths
    lo, _ = wr.interval(im.DEC_KV_LENS, None, im.DEC_B, 3, im.DEC_CAP, im.DEC_W)
    assert (int(lo[2, 0]), int(lo[1, 0])) == (228, 58) and 228 % 64 and 58 % 64
    assert [im.page_size(f, ns) for f in ("_paged", "_paged_kv8") for ns in im.DEC_SPLITS] == [64, 128, 128, 64]


# ---- the cases of a group of cells ----------------------------------------------------------

@functools.lru_cache(maxsize=None)
def decode_cases(variant, d, nb, ty, kv8):
    out = []
    for g, sq in im.decode_geoms(variant, nb):
        kinds = [("census", "random_tree"), ("needle", "own")]
        if variant == "_tree":
            kinds.insert(1, ("census", "arbitrary"))
        out += [im.build(kind, im.decode_shape(variant, d, g, sq, mask), im.DTYPE[ty], kv8) for kind, mask in kinds]
    return out


@functools.lru_cache(maxsize=None)
def packed_cases(family, variant, d, ty, kv8):
    shape = im.attn_shape if family == "fa_attn_varlen" else im.prefill_shape
    return [im.build(kind, shape(variant, d, causal), im.DTYPE[ty], kv8)
            for causal in ((True, False) if variant == "" else (True,)) for kind in ("census", "needle")]


def contract(case):
    """(O, LSE) of the float64 contract the variant's helper module restates."""
    sh = case.shape
    q, k, v = case.dequant()
    if sh.words is not None:
        return tr.contract_f64(q, k, v, tr.vis(sh.words, sh.kv_lens, sh.sq, sh.cap, sh.window), case.sinks)[:2]
    if case.sinks is not None:
        return sr.contract_f64(q, k, v, sh.kv_lens, sh.q_lens, sh.window, case.sinks, sh.causal)[:2]
    if sh.window:
        return wr.contract_f64(q, k, v, sh.kv_lens, sh.q_lens, sh.window)[:2]
    return pr.contract_f64(q, k, v, sh.kv_lens, sh.q_lens, sh.causal)[:2]


def _hold(case, what):
    """The closed form within its own gate of the contract's rounded result, and
    the fault-free model equal to the contract on the written rows."""
    o, lse = contract(case)
    for dtype in im.DTYPE.values():  # (the inputs are exact in both types)
        im.check(case, im.rounded(o, dtype), torch.from_numpy(lse), what, dtype).require()
    mo, ml = im.model(case)
    w = case.rows
    for bi in range(case.shape.b):
        assert np.allclose(mo[bi][:, w[bi]], o[bi][:, w[bi]], rtol=1e-12, atol=1e-14), what
        a, z = ml[bi][:, w[bi]], lse[bi][:, w[bi]]
        assert np.array_equal(np.isneginf(a), np.isneginf(z)), what
        assert np.allclose(a[np.isfinite(z)], z[np.isfinite(z)], rtol=0, atol=1e-11), what


@pytest.mark.parametrize("nb", im.NBS)
@pytest.mark.parametrize("d", im.DIMS)
@pytest.mark.parametrize("variant", im.DECODE_VARIANTS, ids=lambda v: v or "plain")
def test_decode_closed_forms_are_the_contract(variant, d, nb):
    for kv8 in (False, True):
        for case in decode_cases(variant, d, nb, "f16", kv8):
            sh = case.shape
            if case.kind == "census":
                assert all(abs(s) > 0.05 for s in case.score) and case.score[0] != case.score[1]
                assert not case.seen.any(-1).all() or sh.sq == 1, "no row without keys"
            else:
                assert (case.pi.numpy()[case.seen.any(-1)[:, None, :].repeat(sh.hq, 1)] >= 0).all()
            _hold(case, f"decode{variant} d={d} nb={nb} {case.kind} kv8={kv8} Sq={sh.sq}")


@pytest.mark.parametrize("d", im.DIMS)
@pytest.mark.parametrize("variant", im.VARIANTS, ids=lambda v: v or "plain")
@pytest.mark.parametrize("family", ["fa_prefill", "fa_attn_varlen"])
def test_prefill_closed_forms_are_the_contract(family, variant, d):
    for kv8 in (False, True) if family == "fa_prefill" else (False,):
        for case in packed_cases(family, variant, d, "f16", kv8):
            _hold(case, f"{family}{variant} d={d} {case.kind} kv8={kv8} causal={case.shape.causal}")


def test_tree_needle_targets_are_seen_by_their_own_row_only():
    for nb in im.NBS:
        g, sq = im.DEC_GEOM[nb]
        words = im.decode_shape("_tree", 64, g, sq).words  # the census's tree: no element's is the chain
        assert (words != tr.masks("chain", im.DEC_B, sq)).any(1).all()
        case = im.build("needle", im.decode_shape("_tree", 64, g, sq, "own"), im.F16, False)
        for bi, n in enumerate(im.DEC_KV_LENS):
            for t in range(sq):
                key = n - sq + t
                if key >= 0:
                    assert case.seen[bi, :, key].sum() == 1 and case.seen[bi, t, key]
                    assert (case.pi[bi, :, t] == key).all()


# ---- sensitivity ------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _accepted(family, variant, d, nb, kv8, fault, page):
    """{type: whether every run of such a cell passes its gates with the fault in
    the model}.  The inputs are exact in both types, so the model runs once."""
    cases = (decode_cases(variant, d, nb, "f16", kv8) if family == "fa_decode"
             else packed_cases(family, variant, d, "f16", kv8))
    ok = dict.fromkeys(im.TYPES, True)
    for case in cases:
        o, lse = im.model(case, fault, page)
        for ty in [t for t in im.TYPES if ok[t]]:
            dtype = im.DTYPE[ty]
            ok[ty] = im.check(case, im.rounded(o, dtype), torch.from_numpy(lse), fault, dtype).ok
        if not any(ok.values()):
            break
    return ok


def _cell_accepts(cell, fault):
    family = "fa_attn_varlen" if cell.family == "fa_attn_varlen" else "fa_decode" if cell.family == "fa_decode" \
        else "fa_prefill"  # (the packed family runs the padded family's tensors)
    pages = (64, 128) if fault == "table_entries_swapped" else (64,)
    return all(_accepted(family, cell.variant, cell.d, cell.nb, "kv8" in cell.form, fault, page)[cell.ty]
               for page in pages)


@pytest.mark.parametrize("fault", im.FAULTS)
def test_every_fault_fails_the_gates_of_every_cell_it_applies_to(fault):
    cells = [c for c in im.cells() if im.fault_applies(fault, c)]
    assert cells
    accepted = [c for c in cells if _cell_accepts(c, fault)]
    print(f"{fault}: rejected in {len(cells) - len(accepted)} of {len(cells)} cells")
    assert not accepted, [im.entry(c) + f" d={c.d} nb={c.nb}" for c in accepted[:8]]


def test_recorder_forwards_and_records():
    class Lib:
        fa_version = 3

        @staticmethod
        def fa_decode_f16(*a):
            return len(a)

        @staticmethod
        def fa_decode_ws_bytes(*a):
            return 0

    rec = im.Recorder(Lib)
    assert rec.fa_version == 3 and rec.fa_decode_f16(1, 2) == 2 and rec.fa_decode_ws_bytes() == 0
    assert rec.calls == ["fa_decode_f16", "fa_decode_ws_bytes"] and rec.launches() == ["fa_decode_f16"]
    rec.clear()
    assert rec.calls == []
