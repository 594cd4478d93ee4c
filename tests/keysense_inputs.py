"""Inputs whose exact attention output is known in closed form and moves by far
more than the gate when one key is wrong (a helper module, not a test:
`import keysense_inputs` from a test file).  numpy and torch only.

Why: on inputs drawn from [-0.5, 0.5] the softmax is nearly flat, every output
is close to the mean of V and shrinks like 1/sqrt(S), and an absolute 1e-3
gate no longer sees a lost key tile, a stale buffer or a causal diagonal that
is off by one key ("Flat inputs under an absolute gate";
tests/test_keysense_cpu.py prints which faults that comparison accepts).

Census -- who was counted.  Q = K = `level` everywhere (level 0, or 0.25 so
that the running maximum is not zero): every score is the same number, p =
exp2(0) = 1 exactly, P is uniform and O counts the visible keys.  V holds
zeros and ones in one of two layouts:
    tile:    V[j, t] = 1 iff t == (j // 64) % D     (column t = key tile t)
    stripe:  V[j, t] = 1 iff t == j % D
so, in integers and then float64,
    O[i, t] = #{visible keys j of row i with V[j, t] = 1} / #{visible keys},
    LSE[i]  = level^2 * D / sqrt(D) + log(#visible);
a row that sees no key gives O = 0 and LSE = -inf.  The tile layout is used
only where ceil(S / 64) <= D, so that no two key tiles share a column.
Gate on O: relative 2^-10 (fp16) / 2^-7 (bf16) plus 1e-7 absolute: twice the
output type's round-to-nearest bound, since the design allows no error but
the final rounding, an fp32 division and fp32 merges.  Signal: a key wrongly
counted or lost in a tile whose column holds c of the row's n visible keys
moves that column by (n - c) / (c n) relative, which is 1/64 = 2^-6 for a full
tile of a long row and more for a short tile (the diagonal one: c is the
row's position in its block).  The gate is at most half of 2^-6 in both
types; that is a condition and is asserted below, not measured.
Gate on LSE: 1e-5 absolute for level 0, else 2^-10 |score| + 1e-5 (the
project's).

Needle -- who was read.  K[j] is a seeded random +-1 vector, Q[i] = 4 K[pi(i)]
and V[j, t] = +1 if bit (t % 16) of j is set else -1; every value is exact in
fp16, bf16 and E4M3.  Row i's score against its target pi(i) is 4 D / sqrt(D)
(45.3 at D = 128, 32 at D = 64), against every other key about N(0, 4^2), so
the exact output is V[pi(i)] up to a leakage of <= 3e-10 (D = 128, S <= 4160)
or <= 1.7e-5 (D = 64, S = 8192), and the output's sign pattern spells the
index of the key the row read.  Gate on O: |O[i] - V[pi(i)]| <= 1e-3, the
project's; on LSE the project's 2^-10 max|score| + 1e-5 against float64.
Target maps (forward, per head number g = b * H + h, row u of 64-row query
block r):
    sweep:     key tile (u + r + 64 g + shift) mod T_vis at in-tile position
               (7 u + 3 r) mod 64, clipped to the last key; causal: T_vis =
               r + 1 and, on the diagonal tile, the row's own key;
    diagonal:  pi(i) = i (causal only): the last visible key of every row.
Decode rows are the G * Sq query rows of a K/V head (decode_targets).
"""
import math
from dataclasses import dataclass, field

import numpy as np
import torch

TILE = 64
LEVELS = (0.0, 0.25)
LAYOUTS = ("tile", "stripe")
REL_GATE = {torch.float16: 2.0 ** -10, torch.bfloat16: 2.0 ** -7}
ABS_GATE = 1e-7
SIGNAL = 2.0 ** -6       # one wrong key of a full 64-key tile, relative (module docstring)
NEEDLE_GATE = 1e-3
NEEDLE_Q = 4.0

for _gate in REL_GATE.values():
    assert _gate <= SIGNAL / 2, (_gate, SIGNAL)


@dataclass
class Result:
    """What a checker found: ok, the worst error beside its gate (O: relative
    for census, absolute for needle; LSE absolute, None when not checked) and,
    when not ok, a message that names the row."""
    ok: bool
    what: str
    err: float
    gate: float
    lse_err: float = None
    lse_gate: float = None
    msg: str = ""
    o_ok: bool = True
    lse_ok: bool = True
    extra: dict = field(default_factory=dict)

    def line(self):
        s = f"{self.what}: err {self.err:.3e} gate {self.gate:.3e}"
        if self.lse_err is not None:
            s += f" | lse err {self.lse_err:.3e} gate {self.lse_gate:.3e}"
        return s

    def require(self):
        print(self.line())
        assert self.ok, f"{self.what}: {self.msg}"
        return self


def _t64(x, device=None):
    if isinstance(x, np.ndarray):
        x = torch.from_numpy(np.ascontiguousarray(x))
    if device is not None:
        x = x.to(device)
    return x.double()


def _where(flat_index, shape):
    return tuple(int(i) for i in np.unravel_index(int(flat_index), tuple(shape)))


def _name_row(idx):
    """idx: index into [..., row]; the last is the row, the one before the head."""
    if len(idx) >= 3:
        return f"batch {idx[-3]} head {idx[-2]} row {idx[-1]}"
    if len(idx) == 2:
        return f"head {idx[0]} row {idx[1]}"
    return f"row {idx[-1]}"


def _check_lse(got, ref, gate):
    """(ok, err, msg) of an LSE [...] against a float64 reference: the same
    rows are -inf, the others differ by <= gate."""
    got, ref = _t64(got), _t64(ref, got.device)
    empty = torch.isneginf(ref)
    if not torch.equal(torch.isneginf(got), empty):
        i = _where(torch.nonzero((torch.isneginf(got) != empty).flatten())[0, 0], ref.shape)
        return False, float("inf"), f"LSE of {_name_row(i)}: got {float(got[i])}, wanted {float(ref[i])}"
    live = ~empty
    if not bool(live.any()):
        return True, 0.0, ""
    diff = torch.where(live, (got - ref).abs(), torch.zeros_like(ref))
    diff = torch.nan_to_num(diff, nan=float("inf"))
    err = float(diff.max())
    if err <= gate:
        return True, err, ""
    i = _where(diff.argmax(), ref.shape)
    return False, err, (f"LSE of {_name_row(i)}: got {float(got[i]):.6f}, wanted {float(ref[i]):.6f} "
                        f"(exp of the difference: {math.exp(min(50.0, float(got[i] - ref[i]))):.4f} "
                        f"times the keys' weight)")


# ---- census ---------------------------------------------------------------------------

def census_layouts(n_keys, d):
    """The V layouts usable over n_keys keys: tile only while no two tiles share a column."""
    return LAYOUTS if -(-n_keys // TILE) <= d else ("stripe",)


def census_v(n_keys, d, layout, device="cpu"):
    """V [n_keys, D] of zeros and ones (int64)."""
    j = torch.arange(n_keys, device=device)
    if layout == "tile":
        assert -(-n_keys // TILE) <= d, (n_keys, d)
        col = (j // TILE) % d
    else:
        assert layout == "stripe", layout
        col = j % d
    v = torch.zeros((n_keys, d), dtype=torch.int64, device=device)
    v[j, col] = 1
    return v


def census_counts(v01):
    """counts[n, t] = #{j < n : V[j, t] = 1}, int64 [n_keys + 1, D]."""
    return torch.cat([torch.zeros_like(v01[:1]), torch.cumsum(v01, 0)], 0)


def census_expected(counts, vis, level):
    """(O float64 [..., D], LSE float64 [...]) of rows that see the first
    vis[...] keys (int64; <= 0: none)."""
    d = counts.shape[1]
    vis = vis.to(counts.device).long().clamp(min=0)
    o = counts[vis].double() / vis.clamp(min=1).double()[..., None]
    score = level * level * d / math.sqrt(d)
    lse = torch.where(vis > 0, score + torch.log(vis.clamp(min=1).double()),
                      torch.full(vis.shape, float("-inf"), dtype=torch.float64, device=vis.device))
    return o, lse


def census_qkv(q_shape, kv_shape, level, layout, dtype, device="cpu"):
    """q [.., rows, D] and k [.., n_keys, D] filled with `level`, v in `layout`."""
    q = torch.full(q_shape, level, dtype=dtype, device=device)
    k = torch.full(kv_shape, level, dtype=dtype, device=device)
    v01 = census_v(kv_shape[-2], kv_shape[-1], layout, device)
    v = v01.to(dtype).expand(kv_shape).contiguous()
    return q, k, v, census_counts(v01)


def census_lse_gate(level, d):
    return 1e-5 if level == 0 else 2.0 ** -10 * (level * level * d / math.sqrt(d)) + 1e-5


def check_census(o, vis, counts, level, layout, what, lse=None, dtype=None):
    """o [..., rows, D] (16-bit tensor, or float64 values already rounded to
    `dtype`) against the census of rows that see the first vis[..., rows] keys
    (vis broadcastable to o's leading shape)."""
    dtype = dtype or o.dtype
    rel = REL_GATE[dtype]
    got = _t64(o)
    vis = torch.as_tensor(vis).to(got.device).long().expand(got.shape[:-1])
    want, lse_want = census_expected(counts.to(got.device), vis, level)
    tol = rel * want.abs() + ABS_GATE
    tol = torch.where((vis <= 0)[..., None], torch.zeros_like(tol), tol)  # unseen rows: exactly 0
    diff = torch.nan_to_num((got - want).abs(), nan=float("inf"), posinf=float("inf"))
    relerr = torch.where(want > 0, diff / want.clamp(min=1e-300), torch.zeros_like(diff))
    res = Result(True, what, float(relerr.max()) if relerr.numel() else 0.0, rel)
    res.extra["abs_on_zero"] = float(torch.where(want > 0, torch.zeros_like(diff), diff).max()) if diff.numel() else 0.0
    bad = diff > tol
    if bool(bad.any()):
        excess = torch.where(bad, diff / (tol + 1e-30), torch.zeros_like(diff))
        i = _where(excess.argmax(), got.shape)
        n = int(vis[i[:-1]])
        col = "key tile" if layout == "tile" else "keys = t mod D, t ="
        res.ok = res.o_ok = False
        res.msg = (f"{_name_row(i[:-1])} column {i[-1]} ({col} {i[-1]}): got {float(got[i]):.6g} "
                   f"= {float(got[i]) * max(n, 1):.3f} of {n} visible keys, wanted "
                   f"{int(counts[n, i[-1]])} of {n} ({int(bad.sum())} elements past the gate)")
    if lse is not None:
        res.lse_gate = census_lse_gate(level, counts.shape[1])
        ok, res.lse_err, msg = _check_lse(lse, lse_want, res.lse_gate)
        if not ok:
            res.ok = res.lse_ok = False
            res.msg = (res.msg + "; " if res.msg else "") + msg
    return res


# ---- needle ---------------------------------------------------------------------------

def needle_kv(lead_shape, n_keys, d, seed, dtype, device="cpu"):
    """K [*lead, n_keys, D] of seeded +-1 and V [*lead, n_keys, D] spelling the key index."""
    assert n_keys <= 1 << 16, n_keys
    gen = torch.Generator(device=device).manual_seed(seed)
    k = (torch.randint(0, 2, (*lead_shape, n_keys, d), generator=gen, device=device,
                       dtype=torch.int8) * 2 - 1).to(dtype)
    j = torch.arange(n_keys, device=device)[:, None]
    t = torch.arange(d, device=device)[None, :] % 16
    v = (((j >> t) & 1) * 2 - 1).to(dtype).expand(*lead_shape, n_keys, d).contiguous()
    return k, v


def _gather_keys(x, pi, group):
    """x [B, Hkv, n_keys, D] at pi [B, Hq, Sq] (Hq = Hkv * group; < 0 reads key 0) -> [B, Hq, Sq, D]."""
    b, hq, sq = pi.shape
    pi = pi.to(x.device).long().clamp(min=0)
    bi = torch.arange(b, device=x.device)[:, None, None]
    hi = (torch.arange(hq, device=x.device) // group)[None, :, None]
    return x[bi, hi, pi]


def needle_q(k, pi, group=1):
    return (NEEDLE_Q * _gather_keys(k, pi, group)).contiguous()


def needle_expected(v, pi, group=1):
    """V[pi] as float64, zero rows where pi < 0 (the row sees no key)."""
    e = _gather_keys(v, pi, group).double()
    return torch.where((pi.to(v.device) < 0)[..., None], torch.zeros_like(e), e)


def needle_score(d):
    return NEEDLE_Q * d / math.sqrt(d)


def needle_lse_ref(q, k, vis):
    """float64 LSE [B, Hq, Sq] of rows that see the first vis[B, Hq, Sq] keys, by
    K/V head in one matmul (a few rows against the cache: decode shapes)."""
    b, hq, sq, d = q.shape
    hkv, n = k.shape[1], k.shape[2]
    s = (q.double().view(b, hkv, (hq // hkv) * sq, d) @ k.double().transpose(-1, -2)) / math.sqrt(d)
    s = s.view(b, hq, sq, n)
    seen = torch.arange(n, device=q.device)[None, None, None, :] < vis.to(q.device)[..., None]
    return torch.logsumexp(s.masked_fill(~seen, float("-inf")), -1)


def spell(row):
    """(key index, clean) read off a needle output row's sign pattern."""
    row = _t64(row)
    key = int(((row[:16] > 0).long() << torch.arange(16, device=row.device)).sum())
    clean = bool(((row.abs() - 1).abs() <= 0.25).all())
    if clean and row.numel() > 16:
        clean = bool(((row > 0) == (row[torch.arange(row.numel(), device=row.device) % 16] > 0)).all())
    return key, clean


def check_needle(o, want, pi, what, lse=None, lse_ref=None, d=None):
    """o [..., rows, D] against want = needle_expected(...) at the absolute
    1e-3; on a miss, the key the offending row read."""
    got = _t64(o)
    want = want.to(got.device)
    diff = torch.nan_to_num((got - want).abs(), nan=float("inf"), posinf=float("inf"))
    err = float(diff.max()) if diff.numel() else 0.0
    res = Result(err <= NEEDLE_GATE, what, err, NEEDLE_GATE)
    res.o_ok = res.ok
    if not res.ok:
        rows = diff.amax(-1)
        i = _where(rows.argmax(), rows.shape)
        target = int(torch.as_tensor(pi)[i])
        key, clean = spell(got[i])
        nbad = int((rows > NEEDLE_GATE).sum())
        if target < 0:
            read = f"a row that sees no key holds {float(got[i].abs().max()):.3g}"
        elif clean:
            read = f"read key {key}, wanted {target}"
        else:
            read = (f"a mixture (|O - V[{target}]| up to {float(rows[i]):.3g}, signs spell key {key}), "
                    f"wanted {target}")
        res.msg = f"{_name_row(i)}: {read} ({nbad} rows past the gate)"
    if lse is not None:
        res.lse_gate = 2.0 ** -10 * needle_score(d or got.shape[-1]) + 1e-5
        ok, res.lse_err, msg = _check_lse(lse, lse_ref, res.lse_gate)
        if not ok:
            res.ok = res.lse_ok = False
            res.msg = (res.msg + "; " if res.msg else "") + msg
    return res


# ---- target maps ----------------------------------------------------------------------

def sweep_targets(n_heads, s, causal, shift=0):
    """pi int64 [n_heads, s] of the sweep map (module docstring)."""
    i = np.arange(s)
    r, u = i // TILE, i % TILE
    g = np.arange(n_heads)[:, None]
    t_vis = (r + 1) if causal else np.full(s, -(-s // TILE))
    tile = (u + r + TILE * g + shift) % t_vis
    pos = np.broadcast_to((7 * u + 3 * r) % TILE, tile.shape)
    if causal:
        pos = np.where(tile == r, u, pos)
    return np.minimum(tile * TILE + pos, s - 1).astype(np.int64)


def diagonal_targets(n_heads, s):
    return np.broadcast_to(np.arange(s, dtype=np.int64), (n_heads, s)).copy()


def coverage(pis, s, causal):
    """Of a forward launch (or several: a list of pi [n_heads, s]): (every
    (64-row query block, visible key tile) pair holds a needle, the share of
    (16-row group, visible key tile) pairs that do, the missed pairs)."""
    if isinstance(pis, np.ndarray):
        pis = [pis]
    n_tiles = -(-s // TILE)
    out = []
    for rows in (TILE, 16):
        nb = -(-s // rows)
        hit = np.zeros((nb, n_tiles), bool)
        blk = np.arange(s) // rows
        for pi in pis:
            hit[np.broadcast_to(blk, pi.shape), pi // TILE] = True
        last = np.minimum((np.arange(nb) + 1) * rows, s) - 1
        need = (np.arange(n_tiles)[None, :] <= (last // TILE)[:, None]) if causal else np.ones_like(hit)
        out.append((hit, need))
    (hit, need), (hit16, need16) = out
    missed = np.argwhere(need & ~hit)
    return len(missed) == 0, float((hit16 & need16).sum()) / float(need16.sum()), missed


def decode_visible(lens, g, sq, causal):
    """int64 [B, 1, Sq]: how many keys query token t of element b sees
    (bottom-right aligned when causal), >= 0."""
    lens = np.asarray(lens, dtype=np.int64)
    t = np.arange(sq)
    vis = lens[:, None] - sq + t[None, :] + 1 if causal else np.broadcast_to(lens[:, None], (len(lens), sq))
    return np.maximum(vis, 0)[:, None, :]


def decode_targets(lens, hkv, g, sq, causal, shift=0, diagonal=False):
    """pi int64 [B, Hkv * G, Sq] (-1: the row sees no key).  Row n = g_local * Sq
    + t of K/V head c = b * Hkv + kvh targets key tile (n + off + 7 c) mod
    T_vis at position (7 n + 3 shift) mod 64, clipped to its last visible key.
    off = G Sq shift + shift // P: a relaunch moves on by the head's G Sq rows,
    and after the P launches that pass over the longest cache once by one
    more tile, so that a tile which only some rows see (the last one, causal)
    meets one of them.  diagonal: its last visible key."""
    b = len(lens)
    vis = np.broadcast_to(decode_visible(lens, g, sq, causal), (b, hkv * g, sq))
    h = np.arange(hkv * g)[None, :, None]
    n = (h % g) * sq + np.arange(sq)[None, None, :]
    c = np.arange(b)[:, None, None] * hkv + h // g
    t_vis = np.maximum(-(-vis // TILE), 1)
    passes = max(1, -(-int(t_vis.max()) // (g * sq)))
    key = ((n + g * sq * shift + shift // passes + 7 * c) % t_vis) * TILE + (7 * n + 3 * shift) % TILE
    key = np.minimum(key, vis - 1)
    if diagonal:
        key = vis - 1
    return np.where(vis > 0, key, -1).astype(np.int64)


def decode_shifts(lens, hkv, g, sq, causal, limit=512):
    """The shifts 0, 1, ... after which every (element, K/V head, key tile below
    the length) has held a needle."""
    b = len(lens)
    tiles = [-(-int(n) // TILE) for n in lens]
    hit = np.zeros((b, hkv, max(tiles + [1])), bool)
    need = np.arange(hit.shape[2])[None, None, :] < np.array(tiles)[:, None, None]
    need = np.broadcast_to(need, hit.shape)
    bi = np.broadcast_to(np.arange(b)[:, None, None], (b, hkv * g, sq))
    hi = np.broadcast_to((np.arange(hkv * g) // g)[None, :, None], (b, hkv * g, sq))
    shifts = []
    for shift in range(limit):
        if not (need & ~hit).any():
            break
        pi = decode_targets(lens, hkv, g, sq, causal, shift)
        live = pi >= 0
        hit[bi[live], hi[live], pi[live] // TILE] = True
        shifts.append(shift)
    assert not (need & ~hit).any(), ("no coverage", lens, hkv, g, sq, causal)
    return shifts
