"""CPU tests of tests/decode_refs.py itself: the three references that carry
the decode GPU tests (the CPU oracle path, fp32 torch, the float64 LSE) agree
with one another at the project's gates on CPU tensors, and paginate / gather
are inverse to one another -- no GPU.

Measured: O differs by at most 1.22e-4 (gate 1e-3), LSE by at most 4.9e-7
(gates 2.7e-4 to 3.2e-4)."""
import numpy as np
import pytest
import torch

import decode_refs as dr

# (B, Hq, Hkv, Sq, cap, D, lens): a group of 2 with a short element; a group of
# 3 whose causal rows partly see nothing (len 2 < Sq 5); a zero-length element
# and len == Sq
SHAPES = [
    (2, 4, 2, 3, 70, 64, (5, 70)),
    (2, 6, 2, 5, 130, 128, (2, 130)),
    (3, 2, 1, 16, 64, 64, (0, 16, 64)),
]


def _cpu(a):
    return torch.from_numpy(np.array(a, dtype=np.uint16).view(np.int16)).view(torch.float16)


@pytest.mark.parametrize("causal", [True, False], ids=["causal", "noncausal"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s[:6])))
def test_references_agree(shape, causal):
    b, hq, hkv, sq, cap, d, lens = shape
    q, k, v = dr.inputs(b, hq, hkv, sq, cap, d)
    what = f"{shape} causal={causal}"
    o_oracle = dr.oracle_decode(q, k, v, np.array(lens), causal).view(np.float16).astype(np.float32)
    lref, smax = dr.lse_ref(q, k, v, lens, causal)
    o_torch, lse_torch = dr.ref_torch(_cpu(q), _cpu(k), _cpu(v), torch.tensor(lens, dtype=torch.int32),
                                      causal)
    unseen = np.isneginf(lref)
    assert not np.isnan(lref).any() and np.isfinite(o_oracle).all(), what
    # LSE: the same -inf pattern, the rest within 2^-10 * smax + 1e-5
    dr.check_lse(lse_torch, lref, smax, what)
    # O: fp32 torch counts as zero on the rows that see no key
    o_torch = np.where(unseen[..., None], 0.0, o_torch.numpy())
    assert np.isfinite(o_torch).all(), what
    err = float(np.abs(o_oracle - o_torch).max())
    print(f"{what}: max |oracle - fp32 torch| {err:.3e}, {int(unseen.sum())} unseen rows")
    assert err <= dr.GATE_F16, (what, err)
    assert not o_oracle[unseen].any(), what


@pytest.mark.parametrize("page_size", [64, 128])
def test_paginate_gather_round_trip(page_size):
    """Lengths that end inside a page: the gathered cache holds the source's rows
    below each length, and nothing else in the pool is anything but NaN."""
    lens = (5, 130, 200)
    _, k, v = dr.inputs(3, 2, 2, 1, 256, 64)
    tk, tv = _cpu(k), _cpu(v)
    assert not bool((tk.view(torch.int16) == dr.NAN_BITS).any() or (tv.view(torch.int16) == dr.NAN_BITS).any())
    kp, vp, table = dr.paginate(tk, tv, page_size, lens, seed=3)
    used = sum(-(-n // page_size) for n in lens)
    assert kp.shape == (used + 5, 2, page_size, 64) and table.shape == (3, 256 // page_size)
    for src, pool in ((tk, kp), (tv, vp)):
        got = dr.gather(pool, table)
        assert got.shape == src.shape
        for i, n in enumerate(lens):
            assert torch.equal(got[i, :, :n].view(torch.int16), src[i, :, :n].view(torch.int16)), i
        live = sum(lens) * src.shape[1] * src.shape[3]
        assert int((pool.view(torch.int16) != dr.NAN_BITS).sum()) == live
