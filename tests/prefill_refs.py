"""What the prefill test files share (a helper module, imported, never
executed by path): the contract's lengths, the three references of
flash_attention_prefill and the comparison against them.

The references are decode_refs' own, called per batch element with that
element's n_b rows and len_b keys (oracle_decode, ref_torch and lse_ref are
generic in Sq; their bottom-right rule `len - Sq + t` with Sq = n_b is the
contract's off_b + t), plus a plain float64 numpy restatement of the contract
that shares no code with them (tests/test_prefill_cpu.py holds the three
against one another).  The gates are decode_refs': fp16 O 1e-3 against the CPU
oracle, bf16 O 5e-3 against fp32 torch, LSE 2^-10 max|score| + 1e-5.

The staircase inputs at the end (scores that move by a chosen step from one
64-key tile to the next, for tests/test_prefill_ranges_gpu.py) come with their
own float64 reference (contract_f64 on the dequantised cache) and a model of
the roundings the design allows; tests/test_prefill_cpu.py holds the two
within half of each gate.
"""
import math

import numpy as np
import torch

import decode_refs as dr
import keysense_inputs as ks


def n_rows(q_lens, b, sq):
    """n_b of the contract: clamp(q_lens[b], 0, Sq), or Sq."""
    if q_lens is None:
        return [sq] * b
    return [min(max(int(x), 0), sq) for x in q_lens]


def n_keys(kv_lens, b, cap):
    if kv_lens is None:
        return [cap] * b
    return [min(max(int(x), 0), cap) for x in kv_lens]


def visible(kv_lens, q_lens, b, sq, cap, causal):
    """int64 [B, Sq]: vis of the contract for rows t < n_b, -1 for rows t >= n_b."""
    vis = np.full((b, sq), -1, np.int64)
    for bi, (n, ln) in enumerate(zip(n_rows(q_lens, b, sq), n_keys(kv_lens, b, cap))):
        t = np.arange(n)
        vis[bi, :n] = np.clip(ln - n + t + 1, 0, ln) if causal else ln
    return vis


def contract_f64(q, k, v, kv_lens, q_lens, causal, with_smax=False):
    """The contract restated in float64 numpy, one row at a time.  q [B,Hq,Sq,D],
    k, v [B,Hkv,cap,D] float arrays.  Returns (O [B,Hq,Sq,D], LSE [B,Hq,Sq],
    written [B,Sq] bool); unwritten rows are NaN, unseen rows 0 / -inf.
    with_smax: a fourth value, the largest |scaled score| of a visible key (what
    the LSE gate is taken from)."""
    q, k, v = (np.asarray(a, dtype=np.float64) for a in (q, k, v))
    b, hq, sq, d = q.shape
    hkv, cap = k.shape[1], k.shape[2]
    g = hq // hkv
    o = np.full((b, hq, sq, d), np.nan)
    lse = np.full((b, hq, sq), np.nan)
    written = np.zeros((b, sq), bool)
    smax = 0.0
    for bi in range(b):
        n_b = sq if q_lens is None else min(max(int(q_lens[bi]), 0), sq)
        len_b = cap if kv_lens is None else min(max(int(kv_lens[bi]), 0), cap)
        off_b = len_b - n_b
        for t in range(n_b):
            written[bi, t] = True
            vis = min(max(off_b + t + 1, 0), len_b) if causal else len_b
            for h in range(hq):
                if vis == 0:
                    o[bi, h, t] = 0.0
                    lse[bi, h, t] = -np.inf
                    continue
                s = k[bi, h // g, :vis] @ q[bi, h, t] / math.sqrt(d)
                m = s.max()
                smax = max(smax, float(np.abs(s).max()))
                e = np.exp(s - m)
                o[bi, h, t] = (e / e.sum()) @ v[bi, h // g, :vis]
                lse[bi, h, t] = m + math.log(e.sum())
    return (o, lse, written, smax) if with_smax else (o, lse, written)


def oracle_rows(q, k, v, kv_lens, q_lens, causal):
    """CPU-oracle O as uint16 fp16 bits [B,Hq,Sq,D] from uint16 inputs: element b
    through decode_refs.oracle_decode with its n_b rows and len_b keys; rows
    t >= n_b are zeros (and not to be compared)."""
    b, hq, sq, d = q.shape
    cap = k.shape[2]
    out = np.zeros((b, hq, sq, d), np.uint16)
    for bi, (n, ln) in enumerate(zip(n_rows(q_lens, b, sq), n_keys(kv_lens, b, cap))):
        if n:
            out[bi, :, :n] = dr.oracle_decode(q[bi:bi + 1, :, :n], k[bi:bi + 1], v[bi:bi + 1], [ln], causal)[0]
    return out


def torch_rows(q, k, v, kv_lens, q_lens, causal):
    """fp32 torch (O [B,Hq,Sq,D], LSE [B,Hq,Sq]) on the tensors' device, element
    by element through decode_refs.ref_torch; rows t >= n_b are zeros / -inf."""
    b, hq, sq, d = q.shape
    cap = k.shape[2]
    o = torch.zeros((b, hq, sq, d), dtype=torch.float32, device=q.device)
    lse = torch.full((b, hq, sq), float("-inf"), dtype=torch.float32, device=q.device)
    for bi, (n, ln) in enumerate(zip(n_rows(q_lens, b, sq), n_keys(kv_lens, b, cap))):
        if n:
            lt = torch.tensor([ln], dtype=torch.int32, device=q.device)
            oo, ll = dr.ref_torch(q[bi:bi + 1, :, :n], k[bi:bi + 1], v[bi:bi + 1], lt, causal)
            o[bi, :, :n], lse[bi, :, :n] = oo[0], ll[0]
    return o, lse


def lse_rows(q, k, v, kv_lens, q_lens, causal):
    """float64 (LSE [B,Hq,Sq], max |scaled score|) through decode_refs.lse_ref;
    rows t >= n_b are -inf (and not to be compared)."""
    b, hq, sq = q.shape[:3]
    cap = k.shape[2]
    lse = np.full((b, hq, sq), -np.inf)
    smax = 0.0
    for bi, (n, ln) in enumerate(zip(n_rows(q_lens, b, sq), n_keys(kv_lens, b, cap))):
        if n:
            ll, sm = dr.lse_ref(q[bi:bi + 1, :, :n], k[bi:bi + 1], v[bi:bi + 1], [ln], causal)
            lse[bi, :, :n] = ll[0]
            smax = max(smax, sm)
    return lse, smax


def refs(host, dev, kv_lens, q_lens, causal, dtype):
    """(O reference, float64 LSE, max |scaled score|), as decode_refs.refs: fp16
    from the CPU oracle where the host bits are given, else fp32 torch."""
    if dtype is torch.float16 and host is not None:
        ro = oracle_rows(*host, kv_lens, q_lens, causal)
        lref, smax = lse_rows(*host, kv_lens, q_lens, causal)
    else:
        ro = torch_rows(*dev, kv_lens, q_lens, causal)[0]
        lref, smax = lse_rows(*dev, kv_lens, q_lens, causal)
    return ro, lref, smax


def check(out, lse, refs_, q_lens, dtype, what):
    """decode_refs.check on the rows t < n_b of every element (the others are
    not part of the result)."""
    ro, lref, smax = refs_
    b, _, sq = lref.shape
    for bi, n in enumerate(n_rows(q_lens, b, sq)):
        if n == 0:
            continue
        r = ro[bi:bi + 1, :, :n]
        dr.check(out[bi:bi + 1, :, :n], lse[bi:bi + 1, :, :n], (r, lref[bi:bi + 1, :, :n], smax), dtype,
                 f"{what} b={bi}")


# ---- key-sensitivity inputs (keysense_inputs) at the prefill shapes -----------------

KS_B, KS_HQ, KS_HKV, KS_SQ, KS_PREFIX, KS_CAP = 2, 8, 2, 321, 200, 576
KS_Q_LENS = (321, 290)
KS_KV_LENS = tuple(KS_PREFIX + n for n in KS_Q_LENS)


def ks_visible(causal=True):
    """int64 [B, 1, Sq] vis of the contract at the key-sensitivity shape (rows t >= n_b: 0)."""
    vis = visible(KS_KV_LENS, KS_Q_LENS, KS_B, KS_SQ, KS_CAP, causal)
    return torch.from_numpy(np.maximum(vis, 0))[:, None, :]


def ks_census(level, layout, d, dtype, device="cpu"):
    """(q, k, v, counts) of the census at the key-sensitivity shape."""
    return ks.census_qkv((KS_B, KS_HQ, KS_SQ, d), (KS_B, KS_HKV, KS_CAP, d), level, layout, dtype, device)


def ks_needle_targets(kind):
    """pi int64 [B, Hq, Sq].  "diagonal": row t reads its last visible key off_b
    + t.  "sweep": an earlier key, tile (7 t + 3 h) mod (visible tiles) at
    in-tile position (5 t + h) mod 64, clipped to the last visible key.  Rows
    t >= n_b get key 0 (they are not compared)."""
    vis = ks_visible(True).numpy()[:, 0, :]                       # [B, Sq]
    t = np.arange(KS_SQ)[None, None, :]
    h = np.arange(KS_HQ)[None, :, None]
    v3 = np.broadcast_to(vis[:, None, :], (KS_B, KS_HQ, KS_SQ))
    if kind == "diagonal":
        pi = v3 - 1
    else:
        assert kind == "sweep", kind
        tiles = np.maximum(-(-v3 // ks.TILE), 1)
        pi = np.minimum(((7 * t + 3 * h) % tiles) * ks.TILE + (5 * t + h) % ks.TILE, v3 - 1)
    return np.where(v3 > 0, pi, 0).astype(np.int64)


def ks_needle(kind, d, dtype, device="cpu", seed=7):
    """(q, k, v, pi, want) of the needle at the key-sensitivity shape."""
    k, v = ks.needle_kv((KS_B, KS_HKV), KS_CAP, d, seed, dtype, device)
    pi = torch.from_numpy(ks_needle_targets(kind))
    g = KS_HQ // KS_HKV
    return ks.needle_q(k, pi, g), k, v, pi, ks.needle_expected(v, pi, g)


def ks_check_census(o, lse, counts, level, layout, what, dtype=None):
    """check_census on the rows t < n_b of each element."""
    vis = ks_visible(True)
    for bi, n in enumerate(KS_Q_LENS):
        ks.check_census(o[bi, :, :n], vis[bi, :, :n], counts, level, layout, f"{what} b={bi}",
                        lse=None if lse is None else lse[bi, :, :n], dtype=dtype).require()


def ks_check_needle(o, lse, q, k, pi, want, what):
    vis = ks_visible(True)
    lref = ks.needle_lse_ref(q, k, vis.expand(KS_B, KS_HQ, KS_SQ)) if lse is not None else None
    for bi, n in enumerate(KS_Q_LENS):
        ks.check_needle(o[bi, :, :n], want[bi, :, :n], pi[bi, :, :n], f"{what} b={bi}",
                        lse=None if lse is None else lse[bi, :, :n],
                        lse_ref=None if lse is None else lref[bi, :, :n], d=o.shape[-1]).require()


# ---- staircase inputs: every 64-key tile at a score level all rows share -------------
#
# Component 0 of K holds the tile's level (a small integer, exact in fp16, bf16 and
# E4M3), component 0 of Q a constant delta (carry "q"), or 1 with delta in the FP8
# cache's k_scale (carry "scale", beside a non-power-of-two v_scale); V and, in the
# noisy flavour, the other components of Q and K are uniform in [-0.5, 0.5) rounded
# to E4M3 (so exact in all three types), in the clean flavour the other components
# of Q are zero.  A row's maximum then moves by step = delta * log2(e) / sqrt(D)
# log2 units per level: the kernel's lazy rescale (fa_fwd_kernel.hpp: m_ref moves,
# and acc, lacc and l32 are multiplied by alpha, only past a growth of 8) is driven
# from either side of its threshold with the earlier tiles still carrying mass.

ST_B, ST_HQ, ST_HKV, ST_SQ, ST_CAP, ST_TILE = 2, 4, 2, 161, 512, 64
ST_Q_LENS = (161, 97)
ST_KV_LENS = (0 + 161, 200 + 97)
ST_V_SCALE = (0.7, 0.9)
# (step, D) -> delta per K/V head; at most 8 significant bits, none a power of two
ST_DELTA = {
    ("4.5", 128): (35.25, 35.5), ("under8", 128): (62.0, 61.5), ("over8", 128): (63.5, 64.5),
    ("12", 128): (94.0, 95.0),
    ("4.5", 64): (25.0, 24.75), ("under8", 64): (43.75, 43.5), ("over8", 64): (45.0, 45.5),
    ("12", 64): (66.5, 67.0),
}
# name -> (levels over the tiles, step, noisy)
ST_PATTERNS = {
    "asc4.5": ("asc", "4.5", True),      # m_ref moves every second tile, 4 % of the mass one tile back
    "under8": ("asc", "under8", False),  # P up to 2^7.9 before m_ref moves
    "over8": ("asc", "over8", False),    # a rescale at every tile
    "asc12": ("asc", "12", True),
    "desc4.5": ("desc", "4.5", True),    # the maximum in tile 0; later P subnormal in fp16
    "jump": ("jump", "12", True),        # level 0 but for each element's last tile below its length
}


class Staircase:
    """q [B,Hq,Sq,D], k, v [B,Hkv,cap,D] float64 (k, v: what the cache holds, the
    codes of an FP8 one), k_scale, v_scale float64 [Hkv] (the fp32 values; ones with
    carry "q"), levels int [B, cap / 64], delta [Hkv]."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def dequant(self):
        """The cache's values in float64: float64(code) * float64(scale)."""
        return (self.k * self.k_scale[None, :, None, None], self.v * self.v_scale[None, :, None, None])


def _e4m3(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(torch.float8_e4m3fn).double().numpy()


_STAIRS = {}


def staircase(pattern, d, carry="q", b=ST_B, hq=ST_HQ, hkv=ST_HKV, sq=ST_SQ, cap=ST_CAP, kv_lens=ST_KV_LENS,
              seed=3):
    """The staircase inputs of `pattern` (a key of ST_PATTERNS) at head_dim d
    (cached, read-only)."""
    key = (pattern, d, carry, b, hq, hkv, sq, cap, tuple(kv_lens), seed)
    if key in _STAIRS:
        return _STAIRS[key]
    kind, step, noisy = ST_PATTERNS[pattern]
    assert carry in ("q", "scale") and cap % ST_TILE == 0 and hq % hkv == 0
    delta = np.array([ST_DELTA[(step, d)][h % 2] for h in range(hkv)])
    rng = np.random.default_rng(seed)
    nt = cap // ST_TILE
    levels = np.zeros((b, nt), np.int64)
    if kind == "asc":
        levels[:] = np.arange(nt)
    elif kind == "desc":
        levels[:] = -np.arange(nt)
    else:
        for bi, n in enumerate(n_keys(kv_lens, b, cap)):
            if n:
                levels[bi, (n - 1) // ST_TILE] = 1
    assert np.abs(levels).max() <= 8  # exact in E4M3
    v = _e4m3(rng.random((b, hkv, cap, d)) - 0.5)
    k = _e4m3(rng.random((b, hkv, cap, d)) - 0.5)
    k[..., 0] = np.repeat(levels, ST_TILE, axis=1)[:, None, :]
    q = _e4m3(rng.random((b, hq, sq, d)) - 0.5) if noisy else np.zeros((b, hq, sq, d))
    if carry == "q":
        q[..., 0] = np.repeat(delta, hq // hkv)[None, :, None]
        k_scale, v_scale = np.ones(hkv), np.ones(hkv)
    else:
        # delta rides on k_scale: the other components' products q_j * code_j * delta
        # keep their size with q_j scaled by 2^-5
        q *= 2.0 ** -5
        q[..., 0] = 1.0
        k_scale = delta.copy()
        v_scale = np.array([ST_V_SCALE[h % 2] for h in range(hkv)], np.float32).astype(np.float64)
    st = Staircase(q=q, k=k, v=v, k_scale=k_scale, v_scale=v_scale, levels=levels, delta=delta, d=d,
                   pattern=pattern, carry=carry, noisy=noisy, step=delta * math.log2(math.e) / math.sqrt(d))
    for a in (q, k, v, k_scale, v_scale, levels, delta):
        a.setflags(write=False)
    _STAIRS[key] = st
    return st


_ST_CONTRACT = {}


def st_contract(pattern, d, carry, causal):
    """contract_f64 of the staircase at the ST_* shape on the dequantised cache
    (cached): (O, LSE, max |scaled score|).  Both 16-bit types read the same values,
    so one result serves both."""
    key = (pattern, d, carry, bool(causal))
    if key not in _ST_CONTRACT:
        st = staircase(pattern, d, carry)
        o, lse, _, smax = contract_f64(st.q, *st.dequant(), ST_KV_LENS, ST_Q_LENS, causal, with_smax=True)
        for a in (o, lse):
            a.setflags(write=False)
        _ST_CONTRACT[key] = (o, lse, smax)
    return _ST_CONTRACT[key]


def st_model(st, dtype, kv_lens, q_lens, causal):
    """(O rounded to dtype as float64, LSE) of a model of the only roundings the
    design allows: the score scale csc = fp32(log2(e) / sqrt(D)) * k_scale in fp32;
    fp16: Q * csc rounded to fp16 before the products (decode_refs' note), bf16:
    the fp32 scores times csc; V's scale on the normalised row; O rounded to the
    output type.  Everything else in float64, through contract_f64 on inputs that
    give exactly those scores."""
    d = st.d
    g = st.q.shape[1] // st.k.shape[1]
    c32 = np.float32(1.4426950408889634) / np.sqrt(np.float32(d))
    csc = np.repeat((c32 * st.k_scale.astype(np.float32)).astype(np.float32), g)[None, :, None, None]
    if dtype is torch.float16:
        qs = (st.q.astype(np.float32) * csc).astype(np.float16).astype(np.float64)
    else:
        qs = st.q * csc.astype(np.float64)
    # contract_f64 divides by sqrt(D) and works in the natural-log domain
    o, lse, _ = contract_f64(qs * (math.log(2.0) * math.sqrt(d)), st.k, st.dequant()[1], kv_lens, q_lens, causal)
    return torch.from_numpy(o).to(dtype).double().numpy(), lse
