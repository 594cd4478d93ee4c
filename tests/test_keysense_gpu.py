"""GPU tests on inputs where every key counts (tests/keysense_inputs.py: the
census and the needle families, closed-form answers, gates and target maps
are described there; tests/test_keysense_cpu.py shows that the checkers
reject a lost, doubled, stale or mis-masked key tile or key).

Every forward tier and every decode variant runs them:
  * forward, forced: every id of fa_mi355x.configs() that the forced entry
    takes (its own mask, dtype and head_dim; the split_kv configs are not
    forceable and run through flash_attention_fwd_splitkv below) at B=2, H=3,
    S = 1000 (16 key tiles, a 40-key tail, the last query block mostly past S)
    and S = 2112 (33 tiles: an odd count for the two-tiles-per-barrier
    programs, more than one item per head);
  * forward, dispatched: the BOUNDARY shapes of tests/fwd_helpers.py (those
    of test_dispatch_sweep_gpu.py) with S >= 256 through
    flash_attention_fwd (workspace path: split tier,
    pool eligibility) and the workspace-free C entry, and
    flash_attention_fwd_splitkv at num_splits 3 and 8 on (1, 8, 2112);
  * decode: the (G, Sq) x D x dtype matrix of test_decode_matrix_gpu.py at
    B=3, Hkv=2, capacity 4160, lengths (70, 1000, 4160): the contiguous entry
    causal and not at num_splits 1, 2, 3, 7, the paged entry on pages of 64 and
    128 (num_splits 1, 3), both again over an FP8 cache with per-head
    power-of-two scales, and the smallest capacity the plan splits by itself.
    At D = 64 the 4160-key element has 65 key tiles on 64 columns, so the
    census tile layout runs with that length cut to 4096 (the stripe layout,
    the LSE and the needle run at 4160).
Each check prints its worst error beside its gate; a failure names the row and
the key (needle) or the key tile (census).

Measured on an MI355X (worst over all cases): census relative error 4.9e-4
(fp16, gate 9.8e-4) and 3.9e-3 (bf16, gate 7.8e-3) in every forced tier, the
split-KV entry, the C entry and decode (decode bf16 NB=4: 3.7e-3): one
rounding of the output.  The one exception is the causal split tier, reached
only through the Python entry's workspace (1x4x8192x128 causal): 8.8e-4 fp16
and 6.8e-3 bf16, because its pieces store 16-bit normalised partials
 and the merged output is rounded a second time; two
roundings stay inside the gate of twice the bound.  Needle: |O - V[pi]| = 0
everywhere; LSE within 2.4e-6 (census within 1.0e-6).
"""
import numpy as np
import pytest
import torch

import decode_refs as dr
import fa_mi355x
import keysense_inputs as ks
from fwd_helpers import BOUNDARY

pytestmark = pytest.mark.gpu

DEV = "cuda"
FP8 = torch.float8_e4m3fn
TILE = ks.TILE
NAN16 = 0x7fff   # int16 bit pattern: NaN in fp16 and in bf16
NAN8 = 0x7f      # the E4M3 NaN


class _Report:
    """Worst census and needle error per tier / variant, failures collected so
    that every tier is reported before the test fails."""

    def __init__(self):
        self.worst, self.fails = {}, []

    def add(self, tier, family, res):
        w = self.worst.setdefault(tier, {})
        w[family] = max(w.get(family, 0.0), res.err)
        if res.lse_err is not None:
            w[family + "_lse"] = max(w.get(family + "_lse", 0.0), res.lse_err)
        if not res.ok:
            self.fails.append(f"{res.what}: {res.msg}")
            print(f"FAIL {res.line()}\n     {res.msg}")

    def finish(self):
        for tier, w in self.worst.items():
            print("KEYSENSE " + tier + ": " + ", ".join(f"{k} {v:.3e}" for k, v in sorted(w.items())))
        assert not self.fails, "\n".join(self.fails[:20])


# ---- forward ----------------------------------------------------------------------------

def _fwd_census(rep, runs, b, h, s, d, causal, dtype, tag):
    """runs: [(tier, fn(q, k, v) -> o)].  All four census variants."""
    vis = torch.arange(1, s + 1, device=DEV) if causal else torch.full((s,), s, device=DEV)
    for level in ks.LEVELS:
        for layout in ks.census_layouts(s, d):
            q, k, v, counts = ks.census_qkv((b, h, s, d), (b, h, s, d), level, layout, dtype, DEV)
            for tier, fn in runs:
                res = ks.check_census(fn(q, k, v), vis, counts, level, layout,
                                      f"census {tier} {tag} level {level} {layout}")
                print(res.line())
                rep.add(tier, "census_rel", res)


def _fwd_needle(rep, runs, b, h, s, d, causal, dtype, tag, seed=5):
    """The sweep map (relaunched with shifted targets until every (64-row query
    block, visible key tile) pair has held a needle: one launch for every
    shape here but the few whose last block has a row or two) and, causal,
    the diagonal map."""
    k, v = ks.needle_kv((b, h), s, d, seed, dtype, DEV)
    maps, full = [], False
    for shift in range(64):
        maps.append((f"sweep+{shift}", ks.sweep_targets(b * h, s, causal, shift)))
        full, share16, missed = ks.coverage([pi for _, pi in maps], s, causal)
        if full:
            break
    assert full, (tag, missed[:8])
    print(f"needle {tag}: {len(maps)} sweep launch(es), every (query block, key tile) pair holds a "
          f"needle, {100 * share16:.1f} % of the (16-row group, key tile) pairs")
    if causal:
        maps.append(("diagonal", ks.diagonal_targets(b * h, s)))
    for name, pi in maps:
        pit = torch.from_numpy(pi).view(b, h, s).to(DEV)
        q, want = ks.needle_q(k, pit), ks.needle_expected(v, pit)
        for tier, fn in runs:
            res = ks.check_needle(fn(q, k, v), want, pit, f"needle {tier} {tag} {name}")
            print(res.line())
            rep.add(tier, "needle_abs", res)


FORCED_S = (1000, 2112)


@pytest.mark.parametrize("family", ["census", "needle"])
@pytest.mark.parametrize("s", FORCED_S)
@pytest.mark.parametrize("d", [128, 64])
@pytest.mark.parametrize("dtype", dr.DTYPES)
def test_forward_forced(dtype, d, s, family):
    """Every forceable tile config of this dtype and head_dim, with its own mask."""
    b, h = 2, 3
    rep = _Report()
    cfgs = [c for c in fa_mi355x.configs()
            if not c.split_kv and c.head_dim == d and c.dtype == str(dtype).split(".")[1]]
    assert cfgs, (dtype, d)
    for causal in (True, False):
        runs = [(c.name, (lambda q, k, v, c=c: fa_mi355x.flash_attention_fwd(q, k, v, causal=c.causal,
                                                                            config=c.id)))
                for c in cfgs if c.causal == causal]
        tag = f"{dr.name(dtype)} d={d} S={s} causal={causal}"
        (_fwd_census if family == "census" else _fwd_needle)(rep, runs, b, h, s, d, causal, dtype, tag)
    rep.finish()


def _c_entry(q, k, v, causal):
    b, h, s, d = q.shape
    lib = fa_mi355x.load_library()
    o = torch.full_like(q, float("nan"))
    fn = lib.fa_fwd_bf16 if q.dtype is torch.bfloat16 else lib.fa_fwd_f16
    rc = fn(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), b, h, s, d, int(causal),
            torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.fa_status_string(rc)
    return o


DISPATCHED = [sh for sh in BOUNDARY if sh[2] >= 256]


@pytest.mark.parametrize("shape", DISPATCHED, ids=lambda sh: "x".join(map(str, sh)))
def test_forward_dispatched(shape):
    """Whatever tier the dispatcher picks: the Python entry (it brings the
    workspace) and the workspace-free C entry."""
    b, h, s, d, causal, bf16 = shape
    dtype = torch.bfloat16 if bf16 else torch.float16
    tier = "-"
    if d == 128 and not bf16:
        tier = fa_mi355x.configs()[fa_mi355x.select_config(b, h, s, causal)].name
    tag = "x".join(map(str, shape))
    runs = [(f"dispatch py {tag} [{tier}]", lambda q, k, v: fa_mi355x.flash_attention_fwd(q, k, v, causal)),
            (f"dispatch c {tag} [{tier}]", lambda q, k, v: _c_entry(q, k, v, causal))]
    rep = _Report()
    _fwd_census(rep, runs, b, h, s, d, causal, dtype, "")
    _fwd_needle(rep, runs, b, h, s, d, causal, dtype, tag)
    rep.finish()


@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("num_splits", [3, 8])
def test_forward_splitkv(num_splits, causal):
    b, h, s, d = 1, 8, 2112, 128
    runs = [(f"splitkv ns={num_splits} causal={causal}",
             lambda q, k, v: fa_mi355x.flash_attention_fwd_splitkv(q, k, v, causal=causal,
                                                                   num_splits=num_splits))]
    rep = _Report()
    _fwd_census(rep, runs, b, h, s, d, causal, torch.float16, "1x8x2112")
    _fwd_needle(rep, runs, b, h, s, d, causal, torch.float16, "1x8x2112")
    rep.finish()


# ---- decode -----------------------------------------------------------------------------

K_SCALE = (2.0 ** -3, 2.0 ** -2)   # per K/V head: +-1 is stored as +-8 and +-4
V_SCALE = (2.0 ** -3, 2.0 ** -1)


def _pad_rows(x, lens, pattern):
    """Rows past each length hold a NaN bit pattern (x: [B, Hkv, cap, D])."""
    raw = x.view(torch.uint8) if x.dtype is FP8 else x.view(torch.int16)
    for i, n in enumerate(lens):
        raw[i, :, int(n):].fill_(pattern)
    return x


def _grow(x, cap):
    """x [B, Hkv, n, D] with rows appended up to cap (they lie past every length)."""
    if x.shape[2] == cap:
        return x
    return torch.cat([x, x[:, :, :cap - x.shape[2]]], 2).contiguous()


def _launchers(k, v, lens, cache, contig_ns, paged_ns, pages=(64, 128)):
    """[(variant, causal, fn(q) -> (out, lse))] over the clean caches k, v
    [B, Hkv, cap, D]: a 16-bit or FP8 copy whose rows past each length are NaN."""
    cap = k.shape[2]
    tl = torch.tensor(list(lens), dtype=torch.int32, device=DEV)
    kw = {}
    if cache == "kv8":
        ksc = torch.tensor(K_SCALE, dtype=torch.float32, device=DEV)
        vsc = torch.tensor(V_SCALE, dtype=torch.float32, device=DEV)
        k8 = (k.float() / ksc[None, :, None, None]).to(FP8)
        v8 = (v.float() / vsc[None, :, None, None]).to(FP8)
        assert torch.equal(k8.float() * ksc[None, :, None, None], k.float())
        assert torch.equal(v8.float() * vsc[None, :, None, None], v.float())
        kc, vc, kw = k8, v8, {"k_scale": ksc, "v_scale": vsc}
        pattern = NAN8
    else:
        kc, vc, pattern = k.clone(), v.clone(), NAN16
    out = []
    kc, vc = _pad_rows(kc, lens, pattern), _pad_rows(vc, lens, pattern)
    for causal in (True, False):
        for ns in contig_ns:
            out.append((f"contig ns={ns}", causal,
                        lambda q, causal=causal, ns=ns: fa_mi355x.flash_attention_decode(
                            q, kc, vc, tl, causal=causal, return_lse=True, num_splits=ns, **kw)))
    for ps in pages:
        pcap = -(-cap // ps) * ps
        kg, vg = (_pad_rows(_grow(x, pcap), lens, pattern) for x in (kc, vc))
        if cache == "kv8":
            kp, vp, table = dr.paginate(kg.view(torch.uint8), vg.view(torch.uint8), ps, lens, seed=ps)
            kp, vp = kp.view(FP8), vp.view(FP8)
        else:
            kp, vp, table = dr.paginate(kg, vg, ps, lens, seed=ps)
        for ns in paged_ns:
            out.append((f"paged{ps} ns={ns}", True,
                        lambda q, kp=kp, vp=vp, table=table, ns=ns: fa_mi355x.flash_attention_decode_paged(
                            q, kp, vp, table, tl, causal=True, return_lse=True, num_splits=ns, **kw)))
    return out


def _decode_case(rep, dtype, d, g, sq, cache, cap, lens, contig_ns, paged_ns, pages=(64, 128)):
    b, hkv = len(lens), 2
    hq = hkv * g
    nb = dr.nb(g, sq)
    base = f"decode {cache} {dr.name(dtype)} d={d} NB={nb}"
    tag = f"G={g} Sq={sq} cap={cap}"

    def tier(variant):
        return f"{base} {variant.split()[0].rstrip('0123456789')}"

    # census: who was counted
    for level in ks.LEVELS:
        for layout in ks.LAYOUTS:
            n_keys = min(cap, TILE * d) if layout == "tile" else cap
            clens = [min(int(n), n_keys) for n in lens]
            v01 = ks.census_v(n_keys, d, layout, DEV)
            counts = ks.census_counts(v01)
            v = _grow(v01.to(dtype).expand(b, hkv, n_keys, d).contiguous(), cap)
            k = torch.full((b, hkv, cap, d), level, dtype=dtype, device=DEV)
            q = torch.full((b, hq, sq, d), level, dtype=dtype, device=DEV)
            for variant, causal, fn in _launchers(k, v, clens, cache, contig_ns, paged_ns, pages):
                vis = torch.from_numpy(ks.decode_visible(clens, g, sq, causal))
                out, lse = fn(q)
                res = ks.check_census(out, vis, counts, level, layout,
                                      f"census {base} {tag} lens={tuple(clens)} {variant} causal={causal} "
                                      f"level {level} {layout}", lse=lse)
                print(res.line())
                rep.add(tier(variant), "census_rel", res)
    # needle: who was read
    k, v = ks.needle_kv((b, hkv), cap, d, 9, dtype, DEV)
    launch = _launchers(k, v, lens, cache, contig_ns, paged_ns, pages)
    for causal in (True, False):
        shifts = ks.decode_shifts(lens, hkv, g, sq, causal)
        print(f"needle {base} {tag} causal={causal}: {len(shifts)} launches per variant until every "
              f"(K/V head, key tile) pair has held a needle")
        vis = torch.from_numpy(np.broadcast_to(ks.decode_visible(lens, g, sq, causal), (b, hq, sq)).copy())
        maps = [(f"sweep+{sh}", ks.decode_targets(lens, hkv, g, sq, causal, sh)) for sh in shifts]
        if causal:
            maps.append(("diagonal", ks.decode_targets(lens, hkv, g, sq, True, diagonal=True)))
        for name, pi in maps:
            pit = torch.from_numpy(pi).to(DEV)
            q, want = ks.needle_q(k, pit, g), ks.needle_expected(v, pit, g)
            lse_ref = ks.needle_lse_ref(q, k, vis)
            for variant, c, fn in launch:
                if c != causal:
                    continue
                out, lse = fn(q)
                res = ks.check_needle(out, want, pit, f"needle {base} {tag} {variant} causal={causal} {name}",
                                      lse=lse, lse_ref=lse_ref, d=d)
                rep.add(tier(variant), "needle_abs", res)
    for t, w in rep.worst.items():
        if t.startswith(base):
            print(f"{t} {tag}: needle worst {w.get('needle_abs', 0):.3e} gate {ks.NEEDLE_GATE:.0e}, "
                  f"lse {w.get('needle_abs_lse', 0):.3e}")


DECODE_LENS = (70, 1000, 4160)


@pytest.mark.parametrize("g,sq", [(5, 1), (7, 3), (4, 16), (16, 5)])
@pytest.mark.parametrize("d", [128, 64])
@pytest.mark.parametrize("dtype", dr.DTYPES)
@pytest.mark.parametrize("cache", ["kv16", "kv8"])
def test_decode(cache, dtype, d, g, sq):
    """5 / 21 / 64 / 80 rows per K/V head over 2, 16 and 65 key tiles; rows past
    each length are NaN patterns."""
    rep = _Report()
    _decode_case(rep, dtype, d, g, sq, cache, 4160, DECODE_LENS, (1, 2, 3, 7), (1, 3))
    rep.finish()


@pytest.mark.parametrize("d", [128, 64])
@pytest.mark.parametrize("dtype", dr.DTYPES)
@pytest.mark.parametrize("cache", ["kv16", "kv8"])
def test_decode_default_split(cache, dtype, d):
    """num_splits = 0 at the smallest capacity (in key tiles) that the plan cuts
    into more than one piece by itself."""
    g, sq, b, hkv = 5, 1, 3, 2
    cap = next(c for c in range(TILE, 1 << 16, TILE)
               if fa_mi355x.decode_num_splits(b, hkv * g, hkv, sq, c, d) > 1)
    assert cap == TILE or fa_mi355x.decode_num_splits(b, hkv * g, hkv, sq, cap - TILE, d) == 1
    print(f"default split: capacity {cap}, {fa_mi355x.decode_num_splits(b, hkv * g, hkv, sq, cap, d)} pieces")
    rep = _Report()
    _decode_case(rep, dtype, d, g, sq, cache, cap, (70, cap - 63, cap), (0,), (0,), pages=(64,))
    rep.finish()
