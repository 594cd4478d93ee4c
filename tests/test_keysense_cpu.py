"""The tests of the tests: the census and needle checkers of
tests/keysense_inputs.py against a float64 numpy attention model with faults
injected into one query block (no GPU; rows are computed a query block at a
time, never an S x S matrix).

Why this file exists.  The suite's accuracy tests draw inputs from
[-0.5, 0.5] and gate max |O - reference| at 1e-3.  On those inputs the
softmax is nearly flat and every output shrinks like 1 / sqrt(S), so at long
S that comparison accepts kernels that lost a key tile, read a stale buffer or
put the causal diagonal one key off.  test_flat_inputs_accept_faults prints,
for each fault below, max |dO| of the faulted block on such inputs beside the
1e-3 gate.  At both S it accepts the causal mask one key off either way
(5.9e-4 at S = 1000, 1.4e-4 at 4160) and at S = 1000 the padded keys counted
(4.6e-4 to 7.5e-4); what it rejects at S = 4160 it rejects by less than a
factor of 2.5 (a lost tile: 1.5e-3 to 1.8e-3), and DESIGN.md section 5.1 has
the S at which those pass too.

The faults, each in the LAST 64-row query block (causal but for pad; x = the
middle one of its visible key tiles):
    drop         key tile x never read
    dup          key tile x read twice
    stale        tile x's K and V are tile x-1's (a stale buffer)
    kv_mismatch  K of tile x paired with V of tile x-1
    diag-1       row i does not see its own key i
    diag+1       row i also sees key i+1
    pad          the keys past a ragged S, up to the tile's end, counted as
                 zero rows (non-causal, where no diagonal hides them; S =
                 1000 only: 4160 is a multiple of 64)
    overlap      two split pieces [0, x] and [x, T) merged: tile x twice
    gap          two split pieces [0, x) and (x, T) merged: tile x lost
    wrong_page   tile x read from the page of tile x+3 (paged decode)
    zero_scores  every score replaced by 0 (Q K^T ignored)

CAUGHT_BY pins which family rejects which fault, by its O and by its LSE
(the forward entries return no LSE: there only the O columns count).  Census
is blind to K (all its scores are equal whatever is read), so its O cannot
see zero_scores (its LSE does at level 0.25, whose score is not 0); needle's O
is blind to a miscount of keys that carry no weight (dup, overlap, diag+1,
pad), which its LSE sees only where the key counted twice is the needle
itself.  Every fault is rejected by at least one family, and by an O check
wherever the tile layout applies.  It does not at S = 4160, D = 64 (65 tiles
on 64 columns): there a whole tile read twice shows in the LSEs only.  Every
forward shape of tests/test_keysense_gpu.py has ceil(S / 64) <= D, and the
decode entries return the LSE.
"""
import math

import numpy as np
import pytest
import torch

import keysense_inputs as ks

TILE = ks.TILE

SHAPES = [(1000, 64), (1000, 128), (4160, 64), (4160, 128)]
FAULTS = ("drop", "dup", "stale", "kv_mismatch", "diag-1", "diag+1", "pad", "overlap", "gap",
          "wrong_page", "zero_scores")

# fault -> the checks that must reject it, of (census O, census LSE, needle O,
# needle LSE); the others must accept it (the model's only other error is the
# output rounding).  "census O" is the four variants (two levels x two
# layouts, the tile layout where it applies) taken together.
CAUGHT_BY = {
    "drop":        {"census_o", "census_lse", "needle_o", "needle_lse"},
    "dup":         {"census_o", "census_lse", "needle_lse"},
    "stale":       {"census_o", "needle_o", "needle_lse"},
    "kv_mismatch": {"census_o", "needle_o"},
    "diag-1":      {"census_o", "census_lse", "needle_o", "needle_lse"},
    "diag+1":      {"census_o", "census_lse"},
    "pad":         {"census_o", "census_lse"},
    "overlap":     {"census_o", "census_lse", "needle_lse"},
    "gap":         {"census_o", "census_lse", "needle_o", "needle_lse"},
    "wrong_page":  {"census_o", "needle_o", "needle_lse"},
    "zero_scores": {"census_lse", "needle_o", "needle_lse"},
}
# where the tile layout does not apply (65 tiles, 64 columns) the stripe
# layout alone is left, in which every full tile adds one to every column:
# whole tiles lost, doubled or swapped leave O where it was (the LSE and the
# needle still see them)
CAUGHT_BY_STRIPE_ONLY = {
    "drop":        {"census_lse", "needle_o", "needle_lse"},
    "dup":         {"census_lse", "needle_lse"},
    "stale":       {"needle_o", "needle_lse"},
    "kv_mismatch": {"needle_o"},
    "overlap":     {"census_lse", "needle_lse"},
    "gap":         {"census_lse", "needle_o", "needle_lse"},
    "wrong_page":  {"needle_o", "needle_lse"},
}


# ---- the model ------------------------------------------------------------------------

def _plan(fault, t_vis, x):
    """(pieces, diagonal offset, count padded keys, zero scores): a piece is a
    list of (K source tile, V source tile, position tile)."""
    tiles = [(t, t, t) for t in range(t_vis)]
    pieces, off, pad, zero = [tiles], 0, False, False
    if fault == "drop":
        pieces = [tiles[:x] + tiles[x + 1:]]
    elif fault == "dup":
        pieces = [tiles[:x + 1] + tiles[x:]]
    elif fault == "stale":
        pieces = [tiles[:x] + [(x - 1, x - 1, x)] + tiles[x + 1:]]
    elif fault == "kv_mismatch":
        pieces = [tiles[:x] + [(x, x - 1, x)] + tiles[x + 1:]]
    elif fault == "diag-1":
        off = -1
    elif fault == "diag+1":
        off = 1
    elif fault == "pad":
        pad = True
    elif fault == "overlap":
        pieces = [tiles[:x + 1], tiles[x:]]
    elif fault == "gap":
        pieces = [tiles[:x], tiles[x + 1:]]
    elif fault == "wrong_page":
        y = (x + 3) % t_vis
        pieces = [tiles[:x] + [(y, y, x)] + tiles[x + 1:]]
    elif fault == "zero_scores":
        zero = True
    else:
        assert fault is None, fault
    return pieces, off, pad, zero


def model_block(q, k, v, r, causal=True, fault=None):
    """float64 attention of query block r of one head (q, k, v: [S, D]):
    (O [rows, D], LSE [rows]), with `fault` injected."""
    s, d = q.shape
    n_tiles = -(-s // TILE)
    rows = np.arange(r * TILE, min((r + 1) * TILE, s))
    t_vis = min(r + 1, n_tiles) if causal else n_tiles
    x = t_vis // 2
    pieces, off, pad, zero = _plan(fault, t_vis, x)
    if off > 0 and causal and (r + 1) * TILE < s:
        pieces[0].append((r + 1, r + 1, r + 1))
    s_eff = n_tiles * TILE if pad else s
    kp = np.zeros((n_tiles * TILE, d))
    vp = np.zeros((n_tiles * TILE, d))
    kp[:s], vp[:s] = k, v
    c = np.arange(TILE)
    parts = []
    for piece in pieces:
        ksrc = np.concatenate([kp[t * TILE:(t + 1) * TILE] for t, _, _ in piece])
        vsrc = np.concatenate([vp[t * TILE:(t + 1) * TILE] for _, t, _ in piece])
        key = np.concatenate([t * TILE + c for _, _, t in piece])
        sc = q[rows] @ ksrc.T / math.sqrt(d)
        if zero:
            sc = np.zeros_like(sc)
        seen = key[None, :] < s_eff
        if causal:
            seen = seen & (key[None, :] <= rows[:, None] + off)
        sc = np.where(seen, sc, -np.inf)
        m = sc.max(1)
        ms = np.where(np.isfinite(m), m, 0.0)
        p = np.exp(sc - ms[:, None])
        parts.append((m, p.sum(1), p @ vsrc))
    big = np.max([m for m, _, _ in parts], 0)
    bs = np.where(np.isfinite(big), big, 0.0)
    l = sum(np.where(np.isfinite(m), np.exp(m - bs), 0.0) * li for m, li, _ in parts)
    acc = sum(np.where(np.isfinite(m), np.exp(m - bs), 0.0)[:, None] * a for m, _, a in parts)
    with np.errstate(divide="ignore", invalid="ignore"):
        o = np.where(l[:, None] > 0, acc / np.where(l > 0, l, 1.0)[:, None], 0.0)
        lse = np.where(l > 0, bs + np.log(np.where(l > 0, l, 1.0)), -np.inf)
    return o, lse, rows


def _np(t):
    return t.double().numpy()


def _applies(fault, s):
    return not (fault == "pad" and s % TILE == 0)


# ---- what each family says of a fault -------------------------------------------------

HEADS = 2   # needle heads: one head's 64 rows cannot reach all 65 key tiles of S = 4160
_INPUTS = {}
_FAMILY = {}


def _inputs(s, d):
    """The census variants and the needle maps of one shape, as float64 numpy
    (built once, read-only)."""
    if (s, d) not in _INPUTS:
        census = []
        for level in ks.LEVELS:
            for layout in ks.census_layouts(s, d):
                q, k, v, counts = ks.census_qkv((s, d), (s, d), level, layout, torch.float64)
                census.append((level, layout, _np(q), _np(k), _np(v), counts))
        k, v = ks.needle_kv((1, HEADS), s, d, 7, torch.float64)
        needle = {}
        for causal in (True, False):
            maps = [("sweep", ks.sweep_targets(HEADS, s, causal))]
            full, _, missed = ks.coverage(maps[0][1], s, causal)
            assert full, missed
            if causal:
                maps.append(("diagonal", ks.diagonal_targets(HEADS, s)))
            needle[causal] = [(name, pi, _np(ks.needle_q(k, torch.from_numpy(pi)[None])[0]),
                               ks.needle_expected(v, torch.from_numpy(pi)[None])[0]) for name, pi in maps]
        _INPUTS[(s, d)] = (census, _np(k[0]), _np(v[0]), needle)
    return _INPUTS[(s, d)]


def _causal_of(fault):
    return fault != "pad"   # padded keys lie past every causal row's diagonal


def _verdicts(s, d, fault):
    """{dtype: ({check: rejected}, messages)} of the four checks on the
    model's last query block (the model runs once, its output is rounded to
    each type)."""
    if (s, d, fault) in _FAMILY:
        return _FAMILY[(s, d, fault)]
    census, nk, nv, needle = _inputs(s, d)
    causal = _causal_of(fault)
    r = -(-s // TILE) - 1
    out = {dt: ({"census_o": False, "census_lse": False, "needle_o": False, "needle_lse": False}, [])
           for dt in (torch.float16, torch.bfloat16)}

    def note(dt, family, res):
        out[dt][0][family + "_o"] |= not res.o_ok
        out[dt][0][family + "_lse"] |= not res.lse_ok
        if not res.ok:
            out[dt][1].append(f"{res.what}: {res.msg}")

    for level, layout, q, k, v, counts in census:
        o, lse, rows = model_block(q, k, v, r, causal, fault)
        vis = torch.from_numpy(rows + 1) if causal else torch.full((len(rows),), s)
        for dt in out:
            note(dt, "census", ks.check_census(torch.from_numpy(o).to(dt), vis, counts, level, layout,
                                               f"census {level} {layout}", lse=torch.from_numpy(lse)))
    for name, pi, q, want in needle[causal]:
        for h in range(HEADS):
            o, lse, rows = model_block(q[h], nk[h], nv[h], r, causal, fault)
            lse_ref = model_block(q[h], nk[h], nv[h], r, causal, None)[1] if fault else lse
            for dt in out:
                note(dt, "needle", ks.check_needle(
                    torch.from_numpy(o).to(dt)[None], want[h, rows][None], pi[h, rows][None],
                    f"needle {name} head {h}", lse=torch.from_numpy(lse)[None],
                    lse_ref=torch.from_numpy(lse_ref)[None], d=d))
    _FAMILY[(s, d, fault)] = out
    return out


@pytest.mark.parametrize("s,d", SHAPES)
def test_clean_model_passes_every_checker(s, d):
    """The unfaulted model, rounded to fp16 and to bf16, passes census (every
    variant, O and LSE) and needle (both maps, O and LSE): the first, a middle
    and the last query block, causal and not."""
    census, nk, nv, needle = _inputs(s, d)
    n_blocks = -(-s // TILE)
    for causal in (True, False):
        for r in sorted({0, n_blocks // 2, n_blocks - 1}):
            tag = f"S={s} D={d} causal={causal} block {r}"
            for level, layout, q, k, v, counts in census:
                o, lse, rows = model_block(q, k, v, r, causal)
                vis = torch.from_numpy(rows + 1) if causal else torch.full((len(rows),), s)
                for dt in (torch.float16, torch.bfloat16):
                    ks.check_census(torch.from_numpy(o).to(dt), vis, counts, level, layout,
                                    f"clean {dt} census {tag} level {level} {layout}",
                                    lse=torch.from_numpy(lse)).require()
            for name, pi, q, want in needle[causal]:
                h = HEADS - 1
                o, lse, rows = model_block(q[h], nk[h], nv[h], r, causal)
                leak = float(np.abs(o - _np(want[h, rows])).max())
                assert leak <= (3e-10 if d == 128 else 1.7e-5), leak  # before rounding
                for dt in (torch.float16, torch.bfloat16):
                    ks.check_needle(torch.from_numpy(o).to(dt)[None], want[h, rows][None], pi[h, rows][None],
                                    f"clean {dt} needle {name} {tag} (leak {leak:.1e})",
                                    lse=torch.from_numpy(lse)[None], lse_ref=torch.from_numpy(lse)[None],
                                    d=d).require()


@pytest.mark.parametrize("s,d", SHAPES)
def test_every_fault_is_rejected(s, d):
    """For both output types: every fault is rejected by census or by needle
    (by an O check where the tile layout applies), and which checks reject
    which fault is as CAUGHT_BY pins it."""
    stripe_only = ks.census_layouts(s, d) == ("stripe",)
    for dt, (clean, msgs) in _verdicts(s, d, None).items():
        assert not any(clean.values()), (dt, msgs)
        print(f"S={s} D={d} {dt} clean model: accepted by every check")
    for fault in FAULTS:
        if not _applies(fault, s):
            print(f"S={s} D={d} {fault}: does not apply (S is a multiple of {TILE})")
            continue
        for dt, (got, msgs) in _verdicts(s, d, fault).items():
            caught = {name for name, hit in got.items() if hit}
            print(f"S={s} D={d} {dt} {fault}: rejected by {sorted(caught)}")
            for m in msgs[:2]:
                print(f"    {m}")
            assert caught, (fault, dt)
            assert stripe_only or caught & {"census_o", "needle_o"}, (fault, dt, caught)
            want = CAUGHT_BY_STRIPE_ONLY.get(fault, CAUGHT_BY[fault]) if stripe_only else CAUGHT_BY[fault]
            assert caught == want, (fault, dt, sorted(caught), sorted(want))


def test_needle_names_the_key_it_read():
    """A row that read the wrong key is reported with that key's index."""
    s, d = 1000, 128
    k, v = ks.needle_kv((1, 2), s, d, 7, torch.float64)
    pi = ks.sweep_targets(2, s, True)
    pit = torch.from_numpy(pi)[None]
    want = ks.needle_expected(v, pit)
    o = want.clone()
    o[0, 1, 700] = v[0, 1, 123]
    res = ks.check_needle(o.to(torch.float16), want, pit, "spell")
    assert not res.ok and f"head 1 row 700: read key 123, wanted {pi[1, 700]}" in res.msg, res.msg


def test_census_names_the_tile():
    s, d = 1000, 128
    _, _, _, counts = ks.census_qkv((s, d), (s, d), 0.0, "tile", torch.float64)
    vis = torch.arange(1, s + 1)
    want, lse = ks.census_expected(counts, vis, 0.0)
    o = want.clone()
    o[900, 5] = 63.0 / 901
    res = ks.check_census(o.to(torch.float16), vis, counts, 0.0, "tile", "tile", lse=lse)
    assert not res.ok and "row 900 column 5 (key tile 5)" in res.msg and "wanted 64 of 901" in res.msg, res.msg


@pytest.mark.parametrize("s,d", SHAPES)
def test_flat_inputs_accept_faults(s, d, capsys):
    """Printed, not asserted: which of the faults the suite's usual comparison
    (inputs uniform on [-0.5, 0.5], max |O - reference| <= 1e-3) accepts."""
    rng = np.random.default_rng(42)
    q, k, v = (rng.uniform(-0.5, 0.5, (s, d)).astype(np.float16).astype(np.float64) for _ in range(3))
    r = -(-s // TILE) - 1
    ref, _, _ = model_block(q, k, v, r, True)
    with capsys.disabled():
        print(f"\nflat inputs, S={s} D={d}, last query block, largest |O| {np.abs(ref).max():.1e}:")
        for fault in FAULTS:
            if not _applies(fault, s):
                continue
            causal = _causal_of(fault)
            o, _, _ = model_block(q, k, v, r, causal, fault)
            err = float(np.abs(o - (ref if causal else model_block(q, k, v, r, False)[0])).max())
            print(f"    {fault:12s} max|dO| {err:.1e}  {'ACCEPTED' if err <= 1e-3 else 'rejected'} at 1e-3")
