"""What the packed (cu_seqlens) test files share (a helper module, imported,
never executed by path): the contract's (s_b, n_b), pack / unpack between the
token-major [T, H, D] tensors of the packed entries and the padded
[B, H, Smax, D] tensors of fa_prefill_* / fa_cache_append_*, and a Python
restatement of the workgroup map of csrc/fa_varlen_map.hpp.

The references of the packed entries are prefill_refs' own on the unpacked
tensors with q_lens = n (prefill_refs.contract_f64, refs, check and the
key-sensitivity checkers), at decode_refs' gates: no new tolerance.
"""
import numpy as np
import torch

import decode_refs as dr  # noqa: F401  (the gates the unpacked results are held to)
import prefill_refs as pr  # noqa: F401


def spans(cu, total):
    """[(s_b, n_b)] of the contract: s_b = clamp(cu[b], 0, T), e_b = clamp(cu[b + 1], s_b, T)."""
    cu = [int(x) for x in cu]
    out = []
    for b in range(len(cu) - 1):
        s = min(max(cu[b], 0), total)
        e = min(max(cu[b + 1], s), total)
        out.append((s, e - s))
    return out


def cu_of(n, start=0):
    """The prefix sum of the token counts n, from `start`."""
    return [start + int(x) for x in np.concatenate([[0], np.cumsum(n)])]


def pack(x, n, total=None, start=0, fill=None):
    """[B, H, Smax, D] -> [T, H, D]: rows t < n_b of element b at packed rows
    start + sum(n[:b]) + t; the rows of no sequence hold `fill` (None: zeros).
    Works on numpy arrays and torch tensors (bit-preserving: indexing only)."""
    b, h, _, d = x.shape
    total = start + int(sum(n)) if total is None else total
    if isinstance(x, torch.Tensor):
        out = torch.zeros((total, h, d), dtype=x.dtype, device=x.device)
        if fill is not None:
            out.view(torch.int16 if x.element_size() == 2 else torch.uint8).fill_(fill)
    else:
        out = np.zeros((total, h, d), x.dtype) if fill is None else np.full((total, h, d), fill, x.dtype)
    s = start
    for bi, nb in enumerate(n):
        if nb:
            rows = x[bi, :, :nb]
            out[s:s + nb] = rows.permute(1, 0, 2) if isinstance(x, torch.Tensor) else rows.transpose(1, 0, 2)
        s += nb
    return out


def unpack(xp, cu, smax=None, fill=0):
    """[T, H, D] -> [B, H, Smax, D] by the contract's spans (rows t >= n_b hold
    `fill`); also [H, T] (an LSE) -> [B, H, Smax]."""
    lse = xp.dim() == 2 if isinstance(xp, torch.Tensor) else xp.ndim == 2
    total = xp.shape[1] if lse else xp.shape[0]
    sp = spans(cu, total)
    smax = max([n for _, n in sp] + [1]) if smax is None else smax
    if lse:
        shape = (len(sp), xp.shape[0], smax)
    else:
        shape = (len(sp), xp.shape[1], smax, xp.shape[2])
    if isinstance(xp, torch.Tensor):
        out = torch.full(shape, fill, dtype=xp.dtype, device=xp.device)
    else:
        out = np.full(shape, fill, xp.dtype)
    for bi, (s, n) in enumerate(sp):
        if n == 0:
            continue
        if lse:
            out[bi, :, :n] = xp[:, s:s + n]
        elif isinstance(xp, torch.Tensor):
            out[bi, :, :n] = xp[s:s + n].permute(1, 0, 2)
        else:
            out[bi, :, :n] = xp[s:s + n].transpose(1, 0, 2)
    return out


def owned_rows(cu, total):
    """bool [T]: the packed rows that belong to a sequence."""
    own = np.zeros(total, bool)
    for s, n in spans(cu, total):
        own[s:s + n] = True
    return own


# ---- the workgroup map (csrc/fa_varlen_map.hpp), restated ------------------------------

def f_map(cu, total, bt):
    """f(b) = s_b / bt + b for b in [0, B]."""
    return [min(max(int(c), 0), total) // bt + b for b, c in enumerate(cu)]


def num_ids(total, nseq, bt):
    """What the host launches, from shapes alone."""
    return total // bt + nseq


def block_of(cu, total, bt, i):
    """The kernel's decision for virtual block id i: (b, r) or None ("return").
    The bisection of varlen_block(): the count of b in [0, B] with f(b) <= i."""
    nseq = len(cu) - 1
    lo, hi = 0, nseq + 1
    while lo < hi:
        mid = (lo + hi) >> 1
        if min(max(int(cu[mid]), 0), total) // bt + mid <= i:
            lo = mid + 1
        else:
            hi = mid
    if lo == 0 or lo > nseq:
        return None
    b = lo - 1
    s, n = spans(cu, total)[b]
    r = i - (s // bt + b)
    return (b, r) if r < (n + bt - 1) // bt else None
