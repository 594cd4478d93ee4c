"""GPU checks at BASELINE.json's full sizes, where a full CPU oracle pass would
take minutes: sampled heads vs the oracle, and size-independent properties.

* config 5 workload (B=64, H=32, S=4096, causal): 2 GiB per tensor; a sample
  of whole heads (first, last, a middle one, plus heads spread over the batch)
  is checked against the oracle at the 1e-3 gate.
* seq=16384 causal / seq=8192 non-causal (configs 3, 4): sampled heads.
* maximum sizes: single heads of 64k, 128k and 1M tokens (the kernels take
  S <= 8388607 at head_dim 128), sampled query rows (block edges, the middle,
  the last row, random rows) against the oracle's row-sampled entry.
* properties: V = 1 -> O = 1; causal row 0 -> O[0] = V[0]; a batch split into
  shards gives bit-identical results to the unsharded launch (what bench.py's
  multi-GPU sharding relies on); output is deterministic across launches.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import oracle  # noqa: E402
from fwd_helpers import bits as _bits, fa as _fa, rand_half as _rand  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-3


def _check_sampled(b, h, s, causal, heads, seed=1):
    fa = _fa()
    shape = (b, h, s, 128)
    q, k, v = _rand(shape, seed), _rand(shape, seed + 1), _rand(shape, seed + 2)
    o = fa.flash_attention_fwd(q, k, v, causal=causal)
    torch.cuda.synchronize()
    worst = 0.0
    for flat in heads:
        bi, hi = divmod(flat, h)
        sl = (slice(bi, bi + 1), slice(hi, hi + 1))
        qs, ks, vs = (_bits(x[sl]) for x in (q, k, v))
        ref = oracle.attention(qs, ks, vs, causal)
        d = oracle.max_abs_diff(_bits(o[sl]), ref)
        worst = max(worst, d)
        assert d <= TOL, f"head {flat} (b={bi}, h={hi}): max_diff={d}"
    return worst


def _sample_rows(s, n=24, seed=0):
    rng = np.random.default_rng(seed)
    edges = [0, 1, 63, 64, 255, 256, s // 2, s - 257, s - 256, s - 64, s - 2, s - 1]
    return sorted(set(edges) | set(rng.integers(0, s, n).tolist()))


@pytest.mark.parametrize("s,h,causal,head_dim", [(65536, 2, True, 128), (65536, 2, False, 128),
                                                 (131072, 1, False, 128), (131072, 1, True, 128),
                                                 (1 << 20, 1, True, 128), (65536, 1, True, 64)])
def test_max_sequence_sampled_rows(s, h, causal, head_dim):
    fa = _fa()
    shape = (1, h, s, head_dim)
    q, k, v = _rand(shape, 21), _rand(shape, 22), _rand(shape, 23)
    o = fa.flash_attention_fwd(q, k, v, causal=causal)
    torch.cuda.synchronize()
    rows = _sample_rows(s)
    for hi in range(h):
        qs, ks, vs = (_bits(x[0, hi]) for x in (q, k, v))
        ref = oracle.attention_rows(qs, ks, vs, rows, causal)
        got = _bits(o[0, hi])[rows]
        d = oracle.max_abs_diff(got, ref)
        assert d <= TOL, f"S={s} head {hi}: max_diff={d}"


@pytest.mark.parametrize("b,h,s", [(1, 4, 8192), (1, 2, 16384), (1, 8, 4096), (2, 8, 2048)])
def test_long_causal_few_heads_kvquad(b, h, s):
    # the selector sends these causal launches to the KV-quad (four-way key
    # split over long heads) or, at up to one round of 64-row pairs, to the
    # paired tier: sampled rows of every head against the oracle
    fa = _fa()
    cfg = fa.configs()[fa.select_config(b, h, s, True)].name
    assert ("_asm_pair_" if s <= 4096 else "_kvquad_") in cfg, cfg
    shape = (b, h, s, 128)
    q, k, v = _rand(shape, 31), _rand(shape, 32), _rand(shape, 33)
    o = fa.flash_attention_fwd(q, k, v, causal=True)
    torch.cuda.synchronize()
    rows = _sample_rows(s, n=12)
    for bi in range(b):
        for hi in range(h):
            qs, ks, vs = (_bits(x[bi, hi]) for x in (q, k, v))
            ref = oracle.attention_rows(qs, ks, vs, rows, True)
            d = oracle.max_abs_diff(_bits(o[bi, hi])[rows], ref)
            assert d <= TOL, f"b={bi} h={hi}: max_diff={d}"


@pytest.mark.parametrize("dtype,head_dim", [("bfloat16", 128), ("float16", 64), ("bfloat16", 64)])
@pytest.mark.parametrize("b,h,s", [(1, 4, 8192), (1, 8, 4096)])
def test_long_causal_few_heads_kvquad_twins(b, h, s, dtype, head_dim):
    # the same selector path through the bf16 / head_dim-64 twins (no oracle
    # covers them): sampled query rows of every head against an fp32 torch
    # reference of those rows, bf16 at the 5e-3 gate of tests/test_bf16_gpu.py
    fa = _fa()
    tdt = torch.float16 if dtype == "float16" else torch.bfloat16
    shape = (b, h, s, head_dim)
    q, k, v = (_rand(shape, 41 + i).to(tdt) for i in range(3))
    o = fa.flash_attention_fwd(q, k, v, causal=True)
    torch.cuda.synchronize()
    rows = torch.tensor(_sample_rows(s, n=12), device=q.device)
    qs = q[:, :, rows].float()
    sc = qs @ k.float().transpose(-1, -2) / head_dim ** 0.5
    keep = torch.arange(s, device=q.device)[None, :] <= rows[:, None]
    sc = sc.masked_fill(~keep, float("-inf"))
    ref = (torch.softmax(sc, dim=-1) @ v.float())
    tol = TOL if dtype == "float16" else 5e-3
    err = (o[:, :, rows].float() - ref).abs().max().item()
    assert err <= tol, f"{dtype} d{head_dim}: max err {err}"


@pytest.mark.parametrize("b,h,s,causal", [(2048, 32, 33, True), (512, 64, 200, False),
                                           (512, 64, 200, True)])
def test_many_heads_sampled(b, h, s, causal):
    # 32-65k heads of a ragged short sequence: grid / item-index arithmetic
    # at its largest (S=33: 4-wave loop, S=200: persistent tier)
    n = b * h
    _check_sampled(b, h, s, causal, [0, 1, h, n // 2 + 3, n - h, n - 2, n - 1])


def test_config5_full_size_sampled_heads():
    b, h = 64, 32
    n = b * h
    heads = [0, 1, h - 1, n // 2, n // 2 + 7, n - h, n - 1] + list(range(3, n, n // 9))
    _check_sampled(b, h, 4096, True, sorted(set(heads))[:16])


@pytest.mark.parametrize("s,causal", [(16384, True), (8192, False)])
def test_long_sequences_sampled_heads(s, causal):
    _check_sampled(1, 32, s, causal, [0, 31], seed=11)


@pytest.mark.parametrize("causal", [False, True])
def test_ones_value_gives_ones(causal):
    fa = _fa()
    shape = (2, 8, 4096, 128)
    q, k = _rand(shape, 3) * 4, _rand(shape, 4) * 4  # peaked softmax too
    v = torch.ones(shape, dtype=torch.float16, device="cuda")
    o = fa.flash_attention_fwd(q.contiguous(), k.contiguous(), v, causal=causal)
    torch.cuda.synchronize()
    assert torch.max(torch.abs(o.float() - 1.0)).item() <= TOL


def test_causal_first_row_is_first_value():
    fa = _fa()
    shape = (1, 16, 2048, 128)
    q, k, v = _rand(shape, 5), _rand(shape, 6), _rand(shape, 7)
    o = fa.flash_attention_fwd(q, k, v, causal=True)
    torch.cuda.synchronize()
    assert torch.equal(o[:, :, 0, :], v[:, :, 0, :])


@pytest.mark.parametrize("causal", [False, True])
def test_batch_shards_bit_identical(causal):
    fa = _fa()
    shape = (8, 32, 1024, 128)
    q, k, v = _rand(shape, 8), _rand(shape, 9), _rand(shape, 10)
    full = fa.flash_attention_fwd(q, k, v, causal=causal)
    parts = [fa.flash_attention_fwd(q[i:i + 2].contiguous(), k[i:i + 2].contiguous(),
                                    v[i:i + 2].contiguous(), causal=causal)
             for i in range(0, 8, 2)]
    torch.cuda.synchronize()
    # shards may select a different tile config; every config must agree with the
    # oracle, and the same config must be bit-identical
    cat = torch.cat(parts)
    if fa.select_config(8, 32, 1024, causal) == fa.select_config(2, 32, 1024, causal):
        assert torch.equal(full, cat)
    else:
        assert torch.max(torch.abs(full.float() - cat.float())).item() <= 2 * TOL


def test_deterministic():
    fa = _fa()
    shape = (1, 32, 2048, 128)
    q, k, v = _rand(shape, 12), _rand(shape, 13), _rand(shape, 14)
    a = fa.flash_attention_fwd(q, k, v, causal=True)
    b = fa.flash_attention_fwd(q, k, v, causal=True)
    torch.cuda.synchronize()
    assert torch.equal(a, b)


def test_golden_fixtures_on_gpu():
    """GPU output vs the committed oracle fixtures (no oracle run needed)."""
    import os

    fa = _fa()
    gold = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    for name in ("attn_h2_s64_causal", "attn_h2_s64_noncausal", "attn_h2_s256_causal",
                 "attn_h2_s256_noncausal"):
        z = np.load(os.path.join(gold, name + ".npz"))
        t = [torch.from_numpy(z[x].view(np.int16)).view(torch.float16).cuda() for x in "qkv"]
        o = fa.flash_attention_fwd(*t, causal=name.endswith("_causal"))
        torch.cuda.synchronize()
        d = oracle.max_abs_diff(_bits(o), z["o"])
        assert d <= TOL, f"{name}: {d}"


def test_register_report():
    """The reference's register/occupancy report (:711-755): no spills, the
    occupancy each config is designed for."""
    fa = _fa()
    for c in fa.configs():
        a = fa.kernel_attrs(c.id)
        assert a["local_size_bytes"] == 0, (c.name, a)
        assert a["blocks_per_cu"] >= 1, (c.name, a)
        assert a["max_threads_per_block"] >= 64 * c.waves
