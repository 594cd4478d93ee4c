"""The matrix of forward attention kernel instantiations and the closed-form
inputs every cell of it is checked on (a helper module, not a test: `import
instantiation_matrix`).  numpy and torch on the CPU only; the GPU test file
moves what it needs to the device.

A cell is one kernel instantiation under one C entry:
    decode    variant {plain, _win, _sink, _tree} x cache form {"", _paged, _kv8,
              _paged_kv8} x {f16, bf16} x D {64, 128} x NB {1, 2, 4}      192
    prefill   family {fa_prefill, fa_prefill_varlen} x variant {plain, _win,
              _sink} x form x type x D                                        96
    no cache  fa_attn_varlen x variant x type x D                             12
entry() composes a cell's C entry from these fields with its own rule, not
fa_mi355x._entry_name's, so that the two can disagree.

Shapes are the smallest at which these kernels can still go wrong.
  decode: B = 3, Hkv = 2, capacity 320 (5 key tiles; 384 under 128-key pages),
    kv_lens (2, 130, 300): rows that see no key when Sq > 2, a length ending
    mid-tile, a length ending mid-tile in the last tile; NaN bits in every row
    at or past each length.  (G, Sq) per NB: (5, 3) 15 rows NB 1; (7, 3) 21 rows
    NB 2 with a head change inside a 16-row block; (16, 5) 80 rows NB 4 with a
    second, partial row group; the non-tree variants also run (5, 1), the
    serving shape.  W = 70: the lower edge of the first row is key 228 of length
    300 and key 58 of length 130, both mid-tile.  Tree cells: a random tree, and
    arbitrary words once per cell.
  prefill: B = 2, Hq = 4, Hkv = 2, Sq = 130 (two 128-row query blocks, the
    second nearly empty), q_lens (130, 97) behind prefixes of (70, 0) keys, so
    kv_lens (200, 97); capacity 256; W = 65; plain cells causal and not.
  no cache: the prefill tensors packed behind an empty query sequence that has
    7 keys: nq (0, 130, 97), nk (7, 200, 97), the keys from packed row 3 (starts
    3, 10, 210: off the 64 boundary), GQA 2, tails that belong to no sequence.

Inputs (keysense_inputs): the census, where O counts the visible keys and LSE =
score + log n, at non-zero scores that differ per K/V head, with the window, the
per-head sinks (sink_refs.census_sinks) and the tree mask all active where the
variant has them; and the needle, whose output spells the key that was read,
with targets at the lower edge of the row's keys and at its last visible key
(tree: the draft key only the row itself sees).  An FP8 cache holds codes
under the per-head power-of-two scales K_SCALE, V_SCALE, so every product is
exact: census O = v_scale[hkv] count / n at score q k_scale[hkv] k8 D / sqrt(D);
needle Q = (4 / k_scale[hkv]) K8[pi].

Gates are the project's and nothing here widens one: census O relative 2^-10
(fp16) / 2^-7 (bf16) + 1e-7 with rows that see no key exactly zero; needle O
1e-3; LSE 2^-10 max(|score|, |sink|) + 1e-5 against float64 (sink_refs.lse_gate).
check() applies them one K/V head at a time to any set of visible keys, because
the heads' scores and an FP8 cache's v_scale differ per K/V head, which the
variants' own census checkers (one score, V of zeros and ones) do not take.
tests/test_instantiation_matrix_cpu.py holds the expectations against the
float64 contracts and shows that each fault of FAULTS fails them.
"""
import math
from collections import namedtuple

import numpy as np
import torch

import keysense_inputs as ks
import sink_refs as sr
import tree_refs as tr
import window_refs as wr

FP8 = torch.float8_e4m3fn
F16, BF16 = torch.float16, torch.bfloat16
DTYPE = {"f16": F16, "bf16": BF16}
NAN16, NAN8 = 0x7fff, 0x7f

VARIANTS = ("", "_win", "_sink")
DECODE_VARIANTS = VARIANTS + ("_tree",)
FORMS = ("", "_paged", "_kv8", "_paged_kv8")
TYPES = ("f16", "bf16")
DIMS = (64, 128)
NBS = (1, 2, 4)
PREFILL_FAMILIES = ("fa_prefill", "fa_prefill_varlen")

K_SCALE = (2.0 ** -6, 2.0 ** -3)
V_SCALE = (2.0 ** -4, 2.0 ** -8)

Cell = namedtuple("Cell", "family variant form ty d nb")  # nb 0: the family has no NB


def entry(cell):
    """The C entry of a cell, from its fields."""
    stem = "fa_decode_tree" if cell.variant == "_tree" else cell.family + cell.variant
    return stem + cell.form + "_" + cell.ty


def decode_cells():
    return [Cell("fa_decode", v, f, ty, d, nb) for v in DECODE_VARIANTS for f in FORMS for ty in TYPES
            for d in DIMS for nb in NBS]


def prefill_cells():
    return [Cell(fam, v, f, ty, d, 0) for fam in PREFILL_FAMILIES for v in VARIANTS for f in FORMS
            for ty in TYPES for d in DIMS]


def attn_cells():
    return [Cell("fa_attn_varlen", v, "", ty, d, 0) for v in VARIANTS for ty in TYPES for d in DIMS]


def cells():
    return decode_cells() + prefill_cells() + attn_cells()


# ---- shapes ---------------------------------------------------------------------------

# b, hq, hkv, sq, cap, d; kv_lens, q_lens (None: Sq rows each); causal, window (0: none),
# sinks (bool), words (int64 [B, Sq] tree masks, or None)
Shape = namedtuple("Shape", "b hq hkv sq cap d kv_lens q_lens causal window sinks words")

DEC_B, DEC_HKV, DEC_CAP = 3, 2, 320
DEC_KV_LENS = (2, 130, 300)
DEC_GEOM = {1: (5, 3), 2: (7, 3), 4: (16, 5)}  # NB -> (G, Sq)
DEC_SERVING = (5, 1)
DEC_W = 70
DEC_SPLITS = (1, 3)

PRE_B, PRE_HQ, PRE_HKV, PRE_SQ, PRE_CAP = 2, 4, 2, 130, 256
PRE_Q_LENS, PRE_KV_LENS = (130, 97), (200, 97)
PRE_W = 65

ATT_NQ, ATT_NK = (0,) + PRE_Q_LENS, (7,) + PRE_KV_LENS
ATT_TQ, ATT_TK, ATT_K_START = 240, 320, 3


def decode_geoms(variant, nb):
    """The (G, Sq) pairs a decode cell runs."""
    return [DEC_GEOM[nb]] + ([DEC_SERVING] if nb == 1 and variant != "_tree" else [])


def decode_shape(variant, d, g, sq, kind="random_tree"):
    """kind: the tree cells' mask, one of tree_refs.KINDS, or "own": each row sees
    the prefix and its own draft key only (the needle's)."""
    words = None
    if variant == "_tree":
        words = (np.broadcast_to(1 << np.arange(sq, dtype=np.int64), (DEC_B, sq)).copy() if kind == "own"
                 else tr.masks(kind, DEC_B, sq, seed=sq + g))
    return Shape(DEC_B, g * DEC_HKV, DEC_HKV, sq, DEC_CAP, d, DEC_KV_LENS, None, True,
                 DEC_W if variant else 0, variant in ("_sink", "_tree"), words)


def prefill_shape(variant, d, causal=True):
    return Shape(PRE_B, PRE_HQ, PRE_HKV, PRE_SQ, PRE_CAP, d, PRE_KV_LENS, PRE_Q_LENS, causal,
                 PRE_W if variant else 0, variant == "_sink", None)


def attn_shape(variant, d, causal=True):
    return Shape(len(ATT_NQ), PRE_HQ, PRE_HKV, PRE_SQ, PRE_CAP, d, ATT_NK, ATT_NQ, causal,
                 PRE_W if variant else 0, variant == "_sink", None)


def page_size(form, ns):
    """Paged forms alternate 64- and 128-key pages over a cell's runs."""
    return (64, 128)[(FORMS.index(form) // 2 + DEC_SPLITS.index(ns)) % 2]


def visibility(sh):
    """(seen bool [B, Sq, cap], rows bool [B, Sq]): the keys each row sees and the
    rows that are written (t < n_b), from the helpers' statements of the contract."""
    j = np.arange(sh.cap)[None, None, :]
    if sh.words is not None:
        return tr.vis(sh.words, sh.kv_lens, sh.sq, sh.cap, sh.window), np.ones((sh.b, sh.sq), bool)
    lo, hi = wr.interval(sh.kv_lens, sh.q_lens, sh.b, sh.sq, sh.cap, sh.window if sh.causal else 0)
    rows = hi >= 0
    if not sh.causal:
        assert sh.window == 0
        lo = np.zeros_like(lo)
        hi = np.where(rows, np.asarray(sh.kv_lens, np.int64)[:, None], -1)
    return (j >= lo[:, :, None]) & (j < hi[:, :, None]) & rows[:, :, None], rows


# ---- cases ----------------------------------------------------------------------------

class Case:
    """One set of inputs with its closed form: q [B,Hq,Sq,D] of `dtype`; k, v
    [B,Hkv,cap,D] of `dtype`, or E4M3 codes under k_scale, v_scale (float64 [Hkv],
    ones beside a 16-bit cache) when kv8 -- clean, the runners put NaN past the
    lengths; sinks float32 [Hq] or None, m int64 [Hq] the keys a sink weighs as
    (census; 0: none); seen, rows as visibility() gives them.  Census: score
    float64 [Hkv], v01 int64 [cap, D].  Needle: pi int64 [B,Hq,Sq] (-1: no key)."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def scale_tensors(self, device):
        if not self.kv8:
            return {}
        return dict(k_scale=torch.tensor(self.k_scale, dtype=torch.float32, device=device),
                    v_scale=torch.tensor(self.v_scale, dtype=torch.float32, device=device))

    def dequant(self):
        """(q, k, v) float64 numpy, the cache as the kernel reads it: code * scale."""
        return (self.q.double().numpy(), self.k.double().numpy() * self.k_scale[None, :, None, None],
                self.v.double().numpy() * self.v_scale[None, :, None, None])


CENSUS_Q = (0.25, 0.5)  # Q's level per K/V head: the two heads' scores differ in every form
CENSUS_K16, CENSUS_K8 = 0.25, 2.0  # K's level in a 16-bit cache; the code in an FP8 one


def _scales(kv8, hkv):
    if not kv8:
        return np.ones(hkv), np.ones(hkv)
    return (np.array([K_SCALE[h % 2] for h in range(hkv)]), np.array([V_SCALE[h % 2] for h in range(hkv)]))


def census(sh, dtype, kv8):
    g = sh.hq // sh.hkv
    k_scale, v_scale = _scales(kv8, sh.hkv)
    qlev = np.array([CENSUS_Q[h % 2] for h in range(sh.hkv)])
    klev = CENSUS_K8 if kv8 else CENSUS_K16
    score = np.array([wr.census_score(float(qlev[h]), klev * float(k_scale[h]), sh.d) for h in range(sh.hkv)])
    q = torch.from_numpy(np.repeat(qlev, g))[None, :, None, None].expand(sh.b, sh.hq, sh.sq, sh.d).to(dtype).contiguous()
    v01 = ks.census_v(sh.cap, sh.d, "stripe")
    kv = (sh.b, sh.hkv, sh.cap, sh.d)
    k = torch.full(kv, klev, dtype=dtype)
    v = v01.to(dtype).expand(kv).contiguous()
    if kv8:
        k, v = k.to(FP8), v.to(FP8)
    sinks, m = None, torch.zeros(sh.hq, dtype=torch.int64)
    if sh.sinks:
        per = [sr.census_sinks(sh.hq, float(s)) for s in score]
        sinks = torch.cat([per[h][0][h * g:(h + 1) * g] for h in range(sh.hkv)])
        m = per[0][1]
    seen, rows = visibility(sh)
    return Case(kind="census", shape=sh, dtype=dtype, kv8=kv8, q=q, k=k, v=v, k_scale=k_scale, v_scale=v_scale,
                sinks=sinks, m=m, seen=seen, rows=rows, score=score, v01=v01)


def needle_targets(sh, seen):
    """pi [B,Hq,Sq]: the first key the row sees (the window's lower edge) where
    head + token is even, else its last; a tree row always its last, its own
    draft key; -1 where the row sees none."""
    has = seen.any(-1)
    first = seen.argmax(-1)
    last = sh.cap - 1 - seen[:, :, ::-1].argmax(-1)
    h = np.arange(sh.hq)[None, :, None]
    t = np.arange(sh.sq)[None, None, :]
    low = ((h + t) % 2 == 0) & (sh.words is None)
    pi = np.where(low, first[:, None, :], last[:, None, :])
    return np.where(has[:, None, :], pi, -1).astype(np.int64)


def needle(sh, dtype, kv8, seed=11):
    g = sh.hq // sh.hkv
    k_scale, v_scale = _scales(kv8, sh.hkv)
    k, v = ks.needle_kv((sh.b, sh.hkv), sh.cap, sh.d, seed, dtype)
    seen, rows = visibility(sh)
    pi = torch.from_numpy(needle_targets(sh, seen))
    q = ks.needle_q(k, pi, g)
    if kv8:
        q = (q.double() / torch.from_numpy(np.repeat(k_scale, g))[None, :, None, None]).to(dtype)
        k, v = k.to(FP8), v.to(FP8)
    sinks = sr.census_sinks(sh.hq, 0.0)[0] if sh.sinks else None
    return Case(kind="needle", shape=sh, dtype=dtype, kv8=kv8, q=q, k=k, v=v, k_scale=k_scale, v_scale=v_scale,
                sinks=sinks, m=None, seen=seen, rows=rows, pi=pi)


def build(kind, sh, dtype, kv8):
    return census(sh, dtype, kv8) if kind == "census" else needle(sh, dtype, kv8)


# ---- the closed forms and their gates ----------------------------------------------------

def expected(case):
    """(O float64 [B,Hq,Sq,D], LSE float64 [B,Hq,Sq]) of the closed form (needle:
    the LSE of the float64 model); computed once per case."""
    if "_expected" not in case.__dict__:
        case._expected = _expected(case)
    return case._expected


def _expected(case):
    sh = case.shape
    g = sh.hq // sh.hkv
    vs = torch.from_numpy(np.repeat(case.v_scale, g))[None, :, None, None]
    if case.kind == "needle":
        return ks.needle_expected(case.v.double(), case.pi, g) * vs, torch.from_numpy(model(case)[1])
    seen = torch.from_numpy(case.seen)
    cnt = seen.long() @ case.v01                       # [B, Sq, D], in integers
    tot = seen.long().sum(-1)[:, None, :] + case.m[None, :, None]  # [B, Hq, Sq]
    o = vs * cnt[:, None].double() / tot.clamp(min=1).double()[..., None]
    sc = torch.from_numpy(np.repeat(case.score, g))[None, :, None]
    lse = torch.where(tot > 0, sc + torch.log(tot.clamp(min=1).double()), torch.full_like(sc, float("-inf")))
    return o, lse


def lse_gate(case, hk):
    """sink_refs.lse_gate over a K/V head's scores and its heads' sinks."""
    sh = case.shape
    g = sh.hq // sh.hkv
    smax = abs(float(case.score[hk])) if case.kind == "census" else ks.needle_score(sh.d)
    if case.sinks is not None:
        smax = max(smax, float(case.sinks[hk * g:(hk + 1) * g].abs().max()))
    return sr.lse_gate(smax)


def check(case, o, lse, what, dtype=None):
    """A keysense_inputs.Result of o [B,Hq,Sq,D] (a 16-bit tensor, or float64
    values already rounded to `dtype`, default the case's) and lse [B,Hq,Sq]
    against the closed form, over the written rows of every element, one K/V
    head at a time.  The inputs are exact in both 16-bit types, so one case
    serves both: only the rounding of O and its gate differ."""
    sh = case.shape
    g = sh.hq // sh.hkv
    got, gl = ks._t64(o).cpu(), ks._t64(lse).cpu()
    want, lwant = expected(case)
    nkeys = torch.from_numpy(case.seen.sum(-1))
    rel = ks.REL_GATE[dtype or case.dtype]
    res = ks.Result(True, what, 0.0, rel if case.kind == "census" else ks.NEEDLE_GATE, 0.0, 0.0)
    msgs = []
    for bi in range(sh.b):
        n = int(case.rows[bi].sum())
        for hk in range(sh.hkv) if n else ():
            hs = slice(hk * g, (hk + 1) * g)
            x, w = got[bi, hs, :n], want[bi, hs, :n]
            where = f"{what} b={bi} hkv={hk}"
            gate = lse_gate(case, hk)
            if case.kind == "needle":
                r = ks.check_needle(x, w, case.pi[bi, hs, :n], where, gl[bi, hs, :n], lwant[bi, hs, :n], sh.d)
                assert abs(r.lse_gate - gate) < 1e-12, (r.lse_gate, gate)
                err, ok, lerr, lok, msg = r.err, r.o_ok, r.lse_err, r.lse_ok, r.msg
            else:
                tol = rel * w.abs() + ks.ABS_GATE
                tol = torch.where((nkeys[bi, :n] == 0)[None, :, None], torch.zeros_like(tol), tol)  # exactly 0
                diff = torch.nan_to_num((x - w).abs(), nan=float("inf"), posinf=float("inf"))
                err = float(torch.where(w > 0, diff / w.clamp(min=1e-300), torch.zeros_like(diff)).max())
                bad = diff > tol
                ok, msg = not bool(bad.any()), ""
                if not ok:
                    i = ks._where(torch.where(bad, diff / (tol + 1e-30), torch.zeros_like(diff)).argmax(), x.shape)
                    msg = (f"head {hk * g + i[0]} row {i[1]} column {i[2]}: got {float(x[i]):.6g}, wanted "
                           f"{float(w[i]):.6g} of {int(nkeys[bi, i[1]])} visible keys ({int(bad.sum())} elements "
                           f"past the gate)")
                lok, lerr, lmsg = ks._check_lse(gl[bi, hs, :n], lwant[bi, hs, :n], gate)
                msg = "; ".join(s for s in (msg, lmsg) if s)
            res.err, res.lse_err, res.lse_gate = max(res.err, err), max(res.lse_err, lerr), max(res.lse_gate, gate)
            res.o_ok, res.lse_ok = res.o_ok and ok, res.lse_ok and lok
            if msg:
                msgs.append(f"b={bi} hkv={hk}: {msg}")
    res.ok = res.o_ok and res.lse_ok
    res.msg = " | ".join(msgs[:3])
    return res


# ---- a float64 model of the kernels' data path, with faults --------------------------------

FAULTS = ("window_low_key_lost", "causal_key_too_many", "neighbour_heads_sink", "neighbour_rows_tree_word",
          "k_and_v_scale_swapped", "other_heads_scales", "table_entries_swapped", "row_to_head_off_by_one")


def fault_applies(fault, cell):
    """Whether a cell's kernel can have the fault at all."""
    return {"window_low_key_lost": cell.variant != "",
            "causal_key_too_many": True,  # (a plain cell's causal run)
            "neighbour_heads_sink": cell.variant in ("_sink", "_tree"),
            "neighbour_rows_tree_word": cell.variant == "_tree",
            "k_and_v_scale_swapped": "kv8" in cell.form,
            "other_heads_scales": "kv8" in cell.form,
            "table_entries_swapped": "paged" in cell.form,
            "row_to_head_off_by_one": cell.family == "fa_decode"}[fault]


def nan_caches(case):
    """The cache as float64 [B,Hkv,cap,D] (an FP8 one: its codes) with NaN in the
    rows at or past each length, as the runners hand it to the kernels (computed
    once per case, read-only)."""
    if "_nan_caches" not in case.__dict__:
        k, v = case.k.float().numpy().astype(np.float64), case.v.float().numpy().astype(np.float64)
        for bi, n in enumerate(case.shape.kv_lens):
            k[bi, :, int(n):] = np.nan
            v[bi, :, int(n):] = np.nan
        k.setflags(write=False)
        v.setflags(write=False)
        case._nan_caches = (k, v)
    return case._nan_caches


def model(case, fault=None, page=64):
    """(O [B,Hq,Sq,D], LSE [B,Hq,Sq]) float64, unrounded: the softmax over the
    keys each row sees and its head's sink column, the G * Sq rows of a K/V head
    together as decode has them (row r = head r / Sq, token r % Sq), the cache
    read through a block table of `page`-key pages.  fault: one of FAULTS."""
    sh = case.shape
    b, hkv, sq, d = sh.b, sh.hkv, sh.sq, sh.d
    g = sh.hq // hkv
    rows = g * sq
    seen = case.seen
    if fault == "neighbour_rows_tree_word":
        seen = tr.vis(np.roll(sh.words, -1, axis=1), sh.kv_lens, sq, sh.cap, sh.window)
    cap = -(-sh.cap // page) * page
    seen = np.concatenate([seen, np.zeros((b, sq, cap - sh.cap), bool)], -1)
    seen = np.broadcast_to(seen[:, None, None], (b, hkv, g, sq, cap)).reshape(b, hkv, rows, cap).copy()
    sk = np.full(sh.hq, -np.inf) if case.sinks is None else case.sinks.double().numpy()
    if fault == "neighbour_heads_sink":
        sk = np.roll(sk, -1)
    sink = np.broadcast_to(sk.reshape(1, hkv, g, 1), (b, hkv, g, sq)).reshape(b, hkv, rows)
    if fault == "row_to_head_off_by_one":
        nxt = (np.arange(rows) + 1) % rows
        seen, sink = seen[:, :, nxt], sink[:, :, nxt]
    has = seen.any(-1)
    ix = np.nonzero(has)
    if fault == "window_low_key_lost":
        seen[ix + (seen.argmax(-1)[ix],)] = False
    if fault == "causal_key_too_many":
        nxt = np.where(has, cap - seen[..., ::-1].argmax(-1), 0)
        ok = np.nonzero(nxt < cap)
        seen[ok + (nxt[ok],)] = True
    kc, vc = (np.concatenate([x, np.full((b, hkv, cap - sh.cap, d), np.nan)], 2) for x in nan_caches(case))
    if fault == "table_entries_swapped":  # the entries of the two newest pages of every sequence that has two
        for bi, n in enumerate(sh.kv_lens):
            used = -(-int(n) // page)
            if used >= 2:
                a, z = (used - 2) * page, (used - 1) * page
                for x in (kc, vc):
                    x[bi, :, a:a + page], x[bi, :, z:z + page] = x[bi, :, z:z + page].copy(), x[bi, :, a:a + page].copy()
    ksc, vsc = case.k_scale, case.v_scale
    if fault == "k_and_v_scale_swapped":
        ksc, vsc = vsc, ksc
    if fault == "other_heads_scales":
        ksc, vsc = ksc[::-1], vsc[::-1]
    q = case.q.double().numpy().reshape(b, hkv, rows, d)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        s = q @ np.swapaxes(kc * ksc[None, :, None, None], -1, -2) / math.sqrt(d)
        z = np.concatenate([np.where(seen, s, -np.inf), sink[..., None]], -1)
        mx = z.max(-1)
        dead = np.isneginf(mx)
        e = np.exp(z - np.where(dead, 0.0, mx)[..., None])
        tot = e.sum(-1)
        lse = np.where(dead, -np.inf, np.where(dead, 0.0, mx) + np.log(np.where(dead, 1.0, tot)))
        p = e[..., :-1] / np.where(dead, 1.0, tot)[..., None]
        o = p @ np.nan_to_num(vc * vsc[None, :, None, None], nan=0.0)
    return o.reshape(b, sh.hq, sq, d), lse.reshape(b, sh.hq, sq)


def rounded(o, dtype):
    """float64 values rounded to the output type."""
    return torch.from_numpy(np.ascontiguousarray(o)).to(dtype).double()


# ---- what the GPU runners share ---------------------------------------------------------

def pad_nan(t, lens, cap_to=None):
    """A copy of a cache [B,Hkv,cap,D] with NaN bits (0x7f in an FP8 one) in the
    rows at or past each length, the capacity grown to `cap_to` rows of the same."""
    if cap_to is not None and cap_to > t.shape[2]:
        big = torch.empty(t.shape[:2] + (cap_to,) + t.shape[3:], dtype=t.dtype, device=t.device)
        big[:, :, :t.shape[2]] = t
        t = big
    else:
        t = t.clone()
    for i, n in enumerate(lens):
        rows = t[i, :, min(int(n), t.shape[2]):]
        if rows.element_size() == 1:
            rows.view(torch.uint8).fill_(NAN8)
        else:
            rows.view(torch.int16).fill_(NAN16)
    return t


def paginate(k, v, page, lens, seed):
    """decode_refs.paginate (a permuted table, junk filler, NaN elsewhere) of
    caches of any of the three types, the capacity grown to whole pages."""
    import decode_refs as dr

    cap = -(-k.shape[2] // page) * page
    k, v = pad_nan(k, lens, cap), pad_nan(v, lens, cap)
    one = k.dtype is FP8
    if one:
        k, v = k.view(torch.uint8), v.view(torch.uint8)
    kp, vp, table = dr.paginate(k, v, page, lens, seed=seed, filler="junk")
    return (kp.view(FP8), vp.view(FP8), table) if one else (kp, vp, table)


class Recorder:
    """A proxy for fa_mi355x._lib: attribute lookups go to the real library and
    come back wrapped, so that every call appends the entry's name to `calls`.
    fa_mi355x._entry() resolves on _lib at every call, so installing it with
    monkeypatch.setattr(fa_mi355x, "_lib", Recorder(lib)) sees every launch."""

    HELPERS = ("_ws_bytes", "_num_splits")
    FAMILIES = ("fa_decode", "fa_prefill", "fa_attn_varlen")

    def __init__(self, lib):
        self._real = lib
        self.calls = []

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if not callable(fn):
            return fn

        def call(*args):
            self.calls.append(name)
            return fn(*args)
        return call

    def launches(self):
        """The forward families' launch entries among the calls, in order."""
        return [c for c in self.calls if c.startswith(self.FAMILIES) and not c.endswith(self.HELPERS)]

    def clear(self):
        del self.calls[:]
