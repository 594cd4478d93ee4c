"""GPU sweep of tests/instantiation_matrix.py: every forward attention kernel
instantiation -- 192 decode, 96 prefill and 12 no-cache cells -- runs through
the public Python function of its cache form under a recorder that names the C
entry it reached, and is held to the census and needle closed forms directly
(never to another cache form) at the project's gates.  The shapes, inputs,
scales and gates are the helper module's; tests/test_instantiation_matrix_cpu.py
holds them against the float64 contracts and shows which faults they reject.

Decode is parametrised by (variant, type, D, NB) and loops over the four cache
forms and num_splits 1 and 3; prefill by (family, variant, type, D) over the
forms; no-cache by (variant, type, D).  Inputs are built once per group."""
import pytest
import torch

import decode_refs as dr
import fa_mi355x
import instantiation_matrix as im
import tree_refs as tr
import varlen_refs as vr

pytestmark = pytest.mark.gpu

DEV = dr.DEV


def _groups(cells, fields):
    """{key: the cells that share `fields`}: a test's parameters are the keys and
    its inner loops run the group's cells, so a cell of the matrix cannot be left out."""
    out = {}
    for c in cells:
        out.setdefault(tuple(getattr(c, f) for f in fields), []).append(c)
    return out


def _params(groups):
    return dict(argvalues=list(groups), ids=["-".join(str(x or "plain") for x in key) for key in groups])


DECODE = _groups(im.decode_cells(), ("variant", "ty", "d", "nb"))
PREFILL = _groups(im.prefill_cells(), ("family", "variant", "ty", "d"))
NO_CACHE = _groups(im.attn_cells(), ("variant", "ty", "d"))


@pytest.fixture
def rec(monkeypatch):
    r = im.Recorder(fa_mi355x.load_library())
    monkeypatch.setattr(fa_mi355x, "_lib", r)
    return r


def _launched(rec, cell, run):
    """run() under the recorder: the one launch entry it called is the cell's."""
    rec.clear()
    out = run()
    assert rec.launches() == [im.entry(cell)], (cell, rec.launches())
    return out


def _kw(case, sh):
    """What a case passes besides the tensors: the scales, window and sinks."""
    kw = dict(return_lse=True, causal=sh.causal, window=sh.window, **case.scale_tensors(DEV))
    if case.sinks is not None:
        kw["sinks"] = case.sinks.to(DEV)
    return kw


def _lens(vals):
    return dr.lens(vals)


# ---- decode -----------------------------------------------------------------------------------

def _decode_runs(variant, nb):
    """[(kind, (G, Sq), mask kind, arbitrary)]: per geometry a census and a needle;
    a tree cell's census also under arbitrary words."""
    runs = []
    for geom in im.decode_geoms(variant, nb):
        runs += [("census", geom, "random_tree"), ("needle", geom, "own")]
        if variant == "_tree":
            runs.append(("census", geom, "arbitrary"))
    return runs


@pytest.mark.parametrize("key", **_params(DECODE))
def test_decode_cells(rec, key):
    variant, ty, d, nb = key
    dtype = im.DTYPE[ty]
    lens = im.DEC_KV_LENS
    tl = _lens(lens)
    done = set()
    for kind, (g, sq), mask in _decode_runs(variant, nb):
        assert dr.nb(g, sq) == nb
        sh = im.decode_shape(variant, d, g, sq, mask)
        for kv8 in (False, True):
            case = im.build(kind, sh, dtype, kv8)
            q, k, v = case.q.to(DEV), case.k.to(DEV), case.v.to(DEV)
            kw = _kw(case, sh)
            if sh.words is not None:
                kw["tree_mask"] = tr.to_device(sh.words, DEV)
            for fi, cell in enumerate(c for c in DECODE[key] if ("kv8" in c.form) == kv8):
                form = cell.form
                # arbitrary words: once per cell, at the split count the form's index picks
                for ns in im.DEC_SPLITS if mask != "arbitrary" else im.DEC_SPLITS[fi:fi + 1]:
                    if "paged" in form:
                        kp, vp, table = im.paginate(k, v, im.page_size(form, ns), lens, seed=ns + sq)
                        run = lambda: fa_mi355x.flash_attention_decode_paged(q, kp, vp, table, tl, num_splits=ns, **kw)
                    else:
                        kc, vc = im.pad_nan(k, lens), im.pad_nan(v, lens)
                        run = lambda: fa_mi355x.flash_attention_decode(q, kc, vc, tl, num_splits=ns, **kw)
                    o, lse = _launched(rec, cell, run)
                    what = f"{im.entry(cell)} d={d} nb={nb} G={g} Sq={sq} {kind} {mask if sh.words is not None else ''} ns={ns}"
                    im.check(case, o, lse, what).require()
                    if ns > 1:
                        assert dr.ws_counters_zero(), what
                done.add(cell)
    assert done == set(DECODE[key])
    print(f"{len(done)} cells")


# ---- prefill ----------------------------------------------------------------------------------

def _prefill_run(family, form, case, sh, q, k, v, ps):
    """() -> (O [B,Hq,Sq,D], LSE [B,Hq,Sq]) of one prefill cell's public function;
    the packed family runs varlen_refs' packing of the same tensors."""
    kw = _kw(case, sh)
    tl, lens = _lens(sh.kv_lens), sh.kv_lens
    if "paged" in form:
        kp, vp, table = im.paginate(k, v, ps, lens, seed=ps + sh.d)
        cache = (kp, vp, table)
    else:
        cache = (im.pad_nan(k, lens), im.pad_nan(v, lens))
    if family == "fa_prefill":
        fn = fa_mi355x.flash_attention_prefill_paged if "paged" in form else fa_mi355x.flash_attention_prefill
        ql = _lens(sh.q_lens)
        return lambda: fn(q, *cache, tl, ql, **kw)
    fn = fa_mi355x.flash_attention_prefill_varlen_paged if "paged" in form else fa_mi355x.flash_attention_prefill_varlen
    cu = vr.cu_of(sh.q_lens)
    qp = vr.pack(q, sh.q_lens, total=cu[-1] + 5, fill=im.NAN16)  # (5 rows of no sequence)
    tcu = torch.tensor(cu, dtype=torch.int32, device=DEV)

    def run():
        o, lse = fn(qp, *cache, tcu, tl, **kw)
        return vr.unpack(o, cu, sh.sq), vr.unpack(lse, cu, sh.sq, fill=float("-inf"))
    return run


@pytest.mark.parametrize("key", **_params(PREFILL))
def test_prefill_cells(rec, key):
    family, variant, ty, d = key
    dtype = im.DTYPE[ty]
    done = set()
    for ci, causal in enumerate((True, False) if variant == "" else (True,)):
        sh = im.prefill_shape(variant, d, causal)
        for kind in ("census", "needle"):
            for kv8 in (False, True):
                case = im.build(kind, sh, dtype, kv8)
                q, k, v = case.q.to(DEV), case.k.to(DEV), case.v.to(DEV)
                for cell in (c for c in PREFILL[key] if ("kv8" in c.form) == kv8):
                    form = cell.form
                    ps = im.page_size(form, im.DEC_SPLITS[(ci + (kind == "needle")) % 2])  # 64 and 128 in turn
                    o, lse = _launched(rec, cell, _prefill_run(family, form, case, sh, q, k, v, ps))
                    im.check(case, o, lse, f"{im.entry(cell)} d={d} {kind} causal={causal} page={ps}").require()
                    done.add(cell)
    assert done == set(PREFILL[key])
    print(f"{len(done)} cells")


# ---- no cache ---------------------------------------------------------------------------------

@pytest.mark.parametrize("key", **_params(NO_CACHE))
def test_no_cache_cells(rec, key):
    variant, ty, d = key
    dtype = im.DTYPE[ty]
    cell, = NO_CACHE[key]
    cu_q, cu_k = vr.cu_of(im.ATT_NQ), vr.cu_of(im.ATT_NK, im.ATT_K_START)
    assert cu_q[-1] < im.ATT_TQ and cu_k[-1] < im.ATT_TK and all(c % 64 for c in cu_k[:-1])
    tq, tk = (torch.tensor(c, dtype=torch.int32, device=DEV) for c in (cu_q, cu_k))
    for causal in (True, False) if variant == "" else (True,):
        sh = im.attn_shape(variant, d, causal)
        for kind in ("census", "needle"):
            case = im.build(kind, sh, dtype, False)
            qp = vr.pack(case.q.to(DEV), im.ATT_NQ, total=im.ATT_TQ, fill=im.NAN16)
            kp, vp = (vr.pack(x.to(DEV), im.ATT_NK, total=im.ATT_TK, start=im.ATT_K_START, fill=im.NAN16)
                      for x in (case.k, case.v))
            kw = _kw(case, sh)
            o, lse = _launched(rec, cell, lambda: fa_mi355x.flash_attention_varlen(qp, kp, vp, tq, tk, **kw))
            o, lse = vr.unpack(o, cu_q, sh.sq), vr.unpack(lse, cu_q, sh.sq, fill=float("-inf"))
            im.check(case, o, lse, f"{im.entry(cell)} d={d} {kind} causal={causal}").require()
    print("1 cells")


# ---- the parametrisation ------------------------------------------------------------------------

def test_the_parametrisation_covers_every_cell():
    """The groups the three tests above are parametrised by are the matrix's 300
    cells, each once: a decode or prefill group holds the four cache forms."""
    ran = [c for groups in (DECODE, PREFILL, NO_CACHE) for group in groups.values() for c in group]
    assert len(ran) == 300 and sorted(ran) == sorted(im.cells())
    assert (len(DECODE), len(PREFILL), len(NO_CACHE)) == (48, 24, 12)
    assert all(sorted(c.form for c in group) == sorted(im.FORMS) for groups in (DECODE, PREFILL)
               for group in groups.values())
