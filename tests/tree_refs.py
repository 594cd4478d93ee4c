"""What the tree-masked decode test files share (a helper module, imported,
never executed by path): the mask generators, the contract of
include/fa_mi355x_tree.h restated in Python ints as vis[b][t][j], a float64
reference that applies vis (sinks as sink_refs.contract_f64 has them), and the
census expectation over an arbitrary set of visible keys.

The contract.  The Sq query tokens are draft tokens, the last Sq keys of the
cache; with len = clamp(kv_lens[b], 0, cap), base = len - Sq and m_t =
tree_mask[b][t] & ((1 << Sq) - 1):
    draft key i (cache row base + i >= 0): seen by row t iff bit i of m_t;
    prefix key j < base: seen iff W == 0 or j > base + depth_t - W,
        depth_t = max(popcount(m_t) - 1, 0).
Nothing here widens a gate: O at decode_refs.GATE_F16 / GATE_BF16 and LSE at
decode_refs.check_lse's 2^-10 max|score or sink| + 1e-5 against float64; the
census at keysense_inputs' gates.
"""
import math

import numpy as np
import torch

import keysense_inputs as ks

KINDS = ("chain", "star", "binary", "random_tree", "arbitrary")


# ---- masks --------------------------------------------------------------------------

def masks_from_parents(parents):
    """int64 [B, Sq] ancestor masks m_t = (1 << t) | m_parent, one token at a
    time (the loop fa_mi355x.tree_mask_from_parents is checked against)."""
    parents = np.asarray(parents, dtype=np.int64)
    b, sq = parents.shape
    m = np.zeros((b, sq), np.int64)
    for bi in range(b):
        for t in range(sq):
            p = int(parents[bi, t])
            assert -1 <= p < t, (bi, t, p)
            m[bi, t] = (1 << t) | (int(m[bi, p]) if p >= 0 else 0)
    return m


def chain_parents(b, sq, seed=0):
    return np.broadcast_to(np.arange(sq, dtype=np.int64) - 1, (b, sq)).copy()


def star_parents(b, sq, seed=0):
    """Element bi: a chain up to token hub = (bi + seed) % Sq, every later token
    a child of the hub (element 0, seed 0: the root and its children: each
    token sees the root and itself)."""
    out = np.zeros((b, sq), np.int64)
    for bi in range(b):
        hub = (bi + seed) % sq
        out[bi] = [t - 1 if t <= hub else hub for t in range(sq)]
    return out


def binary_parents(b, sq, seed=0):
    """Element bi: the complete (2 + (bi + seed) % 3)-ary tree in level order."""
    out = np.zeros((b, sq), np.int64)
    for bi in range(b):
        arity = 2 + (bi + seed) % 3
        out[bi] = [(t - 1) // arity if t else -1 for t in range(sq)]
    return out


def random_parents(b, sq, seed=0):
    """Seeded: parents[bi, t] uniform in [-1, t) (several roots are allowed)."""
    rng = np.random.default_rng(1000 + seed)
    return np.stack([np.array([int(rng.integers(-1, t)) if t else -1 for t in range(sq)], np.int64)
                     for _ in range(b)])


def arbitrary_words(b, sq, seed=0):
    """Seeded 32-bit words that are no trees: bits from Sq on are set in every
    other word (the contract ignores them), the self bit is often missing, and
    one row of every element is zero (a row that sees no draft key)."""
    rng = np.random.default_rng(2000 + seed)
    m = rng.integers(0, 1 << 32, size=(b, sq), dtype=np.int64)
    low = (1 << sq) - 1
    m[:, ::2] &= low | (0x5a5a << 16)
    m[:, 1::2] &= low
    for bi in range(b):
        m[bi, (bi + seed) % sq] = 0 if bi % 2 == 0 else ~low & 0xffffffff  # zero, or zero below Sq
    return m


def masks(kind, b, sq, seed=0):
    """int64 [B, Sq] words (values in [0, 2^32)) of one of KINDS; they differ
    per batch element."""
    if kind == "arbitrary":
        return arbitrary_words(b, sq, seed)
    parents = {"chain": chain_parents, "star": star_parents, "binary": binary_parents,
               "random_tree": random_parents}[kind](b, sq, seed)
    return masks_from_parents(parents)


def to_device(m, device="cuda"):
    """The int32 [B, Sq] tensor of int64 words (bit 31 becomes the sign)."""
    return torch.from_numpy(np.asarray(m, dtype=np.int64).astype(np.uint32).view(np.int32).copy()).to(device)


# ---- the contract, in Python ints ---------------------------------------------------

def clamp_lens(kv_lens, b, cap):
    return [cap if kv_lens is None else min(max(int(kv_lens[bi]), 0), cap) for bi in range(b)]


def vis(words, kv_lens, sq, cap, window=0):
    """bool [B, Sq, cap]: vis[b][t][j], key j of element b seen by draft token t."""
    b = len(words)
    assert window == 0 or window >= sq, (window, sq)
    out = np.zeros((b, sq, cap), bool)
    for bi, ln in enumerate(clamp_lens(kv_lens, b, cap)):
        base = ln - sq
        for t in range(sq):
            m = int(words[bi][t]) & ((1 << sq) - 1)
            pos = base + max(bin(m).count("1") - 1, 0)
            for j in range(ln):
                if j >= base:
                    out[bi, t, j] = bool((m >> (j - base)) & 1)
                else:
                    out[bi, t, j] = window == 0 or j > pos - window
    return out


def first_visible(kv_lens, b, sq, cap, window):
    """[B]: max(0, len - Sq + 1 - W), below which no row of any mask sees a key
    (W = 0: key 0)."""
    return [max(0, ln - sq + 1 - window) if window else 0 for ln in clamp_lens(kv_lens, b, cap)]


# ---- float64 reference --------------------------------------------------------------

def f64(x):
    """uint16 fp16 bits, a torch tensor or a float array -> float64 numpy."""
    if isinstance(x, torch.Tensor):
        return x.detach().double().cpu().numpy()
    x = np.asarray(x)
    return x.view(np.float16).astype(np.float64) if x.dtype == np.uint16 else x.astype(np.float64)


def contract_f64(q, k, v, seen, sinks=None):
    """(O [B,Hq,Sq,D], LSE [B,Hq,Sq], max |scaled score or finite sink|) in
    float64 numpy: the softmax over the keys `seen` [B,Sq,cap] marks and the
    sink column (sinks [Hq] or None), which meets no value; a row with neither:
    O = 0, LSE = -inf.  One (element, token, K/V head) at a time, its heads
    together."""
    q, k, v = f64(q), f64(k), f64(v)
    b, hq, sq, d = q.shape
    hkv = k.shape[1]
    g = hq // hkv
    sk = np.full(hq, -np.inf) if sinks is None else f64(sinks)
    o = np.zeros((b, hq, sq, d))
    lse = np.full((b, hq, sq), -np.inf)
    finite = np.abs(sk[np.isfinite(sk)])
    smax = float(finite.max()) if finite.size else 0.0
    for bi in range(b):
        for t in range(sq):
            keys = np.nonzero(seen[bi, t])[0]
            for hk in range(hkv):
                hs = slice(hk * g, (hk + 1) * g)
                s = q[bi, hs, t] @ k[bi, hk, keys].T / math.sqrt(d)  # [G, keys]
                if s.size:
                    smax = max(smax, float(np.abs(s).max()))
                z = np.concatenate([s, sk[hs, None]], 1)
                m = z.max(1)
                live = ~np.isneginf(m)
                e = np.exp(z[live] - m[live, None])
                tot = e.sum(1)
                o[bi, hs, t][live] = (e[:, :-1] / tot[:, None]) @ v[bi, hk, keys]
                lse[bi, hs, t][live] = m[live] + np.log(tot)
    return o, lse, smax


def check(out, lse, ref, seen, gate, what):
    """|O - ref| <= gate, O finite and exactly zero on rows that see no key, and
    decode_refs.check_lse's gate on the LSE (-inf exactly where the reference
    has it)."""
    import decode_refs as dr

    ro, lref, smax = ref
    got = f64(out)
    assert np.isfinite(got).all(), what
    err = float(np.abs(got - ro).max())
    print(f"{what}: max_abs_diff {err:.3e} gate {gate:.1e}")
    assert err <= gate, (what, err, gate)
    nokey = ~np.asarray(seen).any(-1)  # [B, Sq]
    assert not got[np.broadcast_to(nokey[:, None, :], got.shape[:-1])].any(), what
    dr.check_lse(lse, lref, smax, what)


# ---- census over an arbitrary set of keys --------------------------------------------

def census_expected(v01, seen, score, m=None):
    """(O float64 [B,Hq,Sq,D], LSE float64 [B,Hq,Sq], n int64 [B,Sq]) of rows
    whose visible keys `seen` [B,Sq,cap] all score `score`: O counts the
    visible keys with a one in each column over their number n (plus m[h], a
    sink worth m keys, in the denominator: sink_refs.census_sinks)."""
    seen = torch.as_tensor(np.asarray(seen))
    cnt = seen.long() @ v01.long()  # [B, Sq, D], in integers
    n = seen.long().sum(-1)        # [B, Sq]
    mm = torch.zeros(1, dtype=torch.long) if m is None else torch.as_tensor(m).long()
    tot = (n[:, None, :] + mm[None, :, None]).double()  # [B, Hq or 1, Sq]
    o = cnt[:, None].double() / tot.clamp(min=1)[..., None]
    lse = torch.where(tot > 0, score + torch.log(tot.clamp(min=1)), torch.full_like(tot, float("-inf")))
    return o, lse, n


def check_census(out, lse, v01, seen, score, what, m=None, lse_gate=None):
    """keysense_inputs.check_census for any set of visible keys: O within
    REL_GATE[dtype] relative + ABS_GATE of the census (rows that see no key
    exactly zero), LSE within lse_gate (default 2^-10 |score| + 1e-5), and the
    visible-key count read back from both exact for every row: round(exp(LSE -
    score)) = n (+ m) and round(O n) = the per-column counts."""
    hq = out.shape[1]
    want, lse_want, n = census_expected(v01, seen, score, m)
    want, lse_want = want.expand(-1, hq, -1, -1), lse_want.expand(-1, hq, -1)
    got = ks._t64(out).cpu()
    rel = ks.REL_GATE[out.dtype]
    tol = rel * want.abs() + ks.ABS_GATE
    tol = torch.where((n == 0)[:, None, :, None], torch.zeros_like(tol), tol)
    diff = torch.nan_to_num((got - want).abs(), nan=float("inf"), posinf=float("inf"))
    bad = diff > tol
    if bool(bad.any()):
        i = ks._where(torch.where(bad, diff / (tol + 1e-30), torch.zeros_like(diff)).argmax(), got.shape)
        raise AssertionError(f"{what}: {ks._name_row(i[:-1])} column {i[-1]}: got {float(got[i]):.6g}, wanted "
                             f"{float(want[i]):.6g} of {int(n[i[0], i[2]])} visible keys "
                             f"({int(bad.sum())} elements past the gate)")
    gate = 2.0 ** -10 * abs(score) + 1e-5 if lse_gate is None else lse_gate
    ok, err, msg = ks._check_lse(lse.cpu(), lse_want, gate)
    assert ok, f"{what}: {msg}"
    mm = torch.zeros(1, dtype=torch.long) if m is None else torch.as_tensor(m).long()
    tot = (n[:, None, :] + mm[None, :, None]).expand(-1, hq, -1)
    live = tot > 0
    back = torch.round(torch.exp(lse.double().cpu() - score))
    assert torch.equal(back[live].long(), tot[live]), f"{what}: a key count read back from the LSE is off"
    cnt = torch.round(got * tot.double()[..., None]).long()
    want_cnt = (torch.as_tensor(np.asarray(seen)).long() @ v01.long())[:, None].expand(-1, hq, -1, -1)
    assert torch.equal(cnt, want_cnt), f"{what}: a per-column key count read back from O is off"
    print(f"{what}: census exact, lse err {err:.3e} gate {gate:.3e}")
