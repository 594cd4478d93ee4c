"""CPU tests of the prefill entries (no GPU): the eight symbols are exported
and declared, their argument statuses (all returned before any launch, so
fake pointers suffice), the Python wrappers' rejections on CPU tensors, the
compile-time resource usage of the four prefill units, the references of
tests/prefill_refs.py against one another in the range decode never reached
(ragged Sq > 16), and the key-sensitivity checkers on the float64 restatement
of the contract at the GPU test's exact shapes, and the staircase inputs of
tests/test_prefill_ranges_gpu.py: the side of the rescale threshold their steps
lie on, exactness in every type, and the references alone against half of
each gate.
"""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import capi_checks as cc
import decode_refs as dr
import fa_mi355x
import fp8_contract  # noqa: F401  (the E4M3 contract the kv8 caches follow; imported as a module)
import keysense_inputs as ks
import prefill_refs as pr

FP8 = torch.float8_e4m3fn
ENTRIES = [(paged, kv8, bf16) for paged in (False, True) for kv8 in (False, True) for bf16 in (False, True)]
SYMBOLS = ["fa_prefill" + ("_paged" if p else "") + ("_kv8" if k else "") + ("_bf16" if b else "_f16")
           for p, k, b in ENTRIES]
INT_MAX = cc.INT_MAX
P = ctypes.c_void_p(0x1000)
err = fa_mi355x.FlashAttentionError


def test_symbols_exported_and_declared():
    assert len(set(SYMBOLS)) == 8
    cc.assert_exported(SYMBOLS)


def _call(entry, q, k, v, o, b, hq, hkv, sq, cap, d, lens=None, qlens=None, causal=1, table=P, npages=100,
          psz=128, mpp=None):
    """One of the eight entries on the shared arguments; the paged ones take
    `cap` as max_pages_per_seq = cap // psz pages of psz keys (or `mpp`)."""
    paged, kv8, bf16 = entry
    fn = getattr(fa_mi355x.load_library(), SYMBOLS[ENTRIES.index(entry)])
    tail = (None, None) if kv8 else ()
    if paged:
        pages = cap // psz if mpp is None and psz > 0 else (mpp or 0)
        return fn(q, k, v, o, None, b, hq, hkv, sq, d, npages, psz, table, pages, lens, qlens, causal, None,
                  *tail)
    return fn(q, k, v, o, None, b, hq, hkv, sq, cap, d, lens, qlens, causal, None, *tail)


@pytest.mark.parametrize("entry", ENTRIES, ids=SYMBOLS)
def test_argument_statuses(entry):
    """The status table of include/fa_mi355x.h.  Every call here returns before
    any launch: an argument error, an empty problem, or -- where a shape must be
    shown to be ACCEPTED -- the NULL q that is looked at after every shape."""
    fa = fa_mi355x
    paged = entry[0]
    call = lambda *a, **kw: _call(entry, *a, **kw)  # noqa: E731
    for bad in range(4):  # each of q, k, v, o NULL in turn
        ptrs = [None if i == bad else P for i in range(4)]
        assert call(*ptrs, 1, 8, 2, 300, 1024, 128) == fa.FA_ERR_NULL_POINTER
    for d in (0, 32, 96, 256):
        assert call(P, P, P, P, 1, 8, 2, 300, 1024, d) == fa.FA_ERR_UNSUPPORTED_HEAD_DIM
    for hq, hkv in ((8, 3), (7, 2), (4, 8)):
        assert call(P, P, P, P, 1, hq, hkv, 300, 1024, 128) == fa.FA_ERR_BAD_SHAPE
    for sq in (0, -1):
        assert call(P, P, P, P, 1, 8, 2, sq, 1024, 128) == fa.FA_ERR_BAD_SHAPE
    # no upper bound on seqlen_q but the 32-bit ranges: these pass every shape check
    for sq in (1, 16, 17, 4096, 1 << 20):
        assert call(None, P, P, P, 1, 8, 2, sq, 1024, 128) == fa.FA_ERR_NULL_POINTER, sq
    assert call(P, P, P, P, -1, 8, 2, 300, 1024, 128) == fa.FA_ERR_BAD_SHAPE
    assert call(P, P, P, P, 1, -8, 2, 300, 1024, 128) == fa.FA_ERR_BAD_SHAPE
    assert call(P, P, P, P, 1, 8, -2, 300, 1024, 128) == fa.FA_ERR_BAD_SHAPE
    # seqlen_q * 2 * head_dim past INT_MAX; batch * heads_q * seqlen_q past INT_MAX
    assert call(P, P, P, P, 1, 1, 1, 1 << 23, 1024, 128) == fa.FA_ERR_BAD_SHAPE
    assert call(None, P, P, P, 1, 1, 1, (1 << 23) - 1, 1024, 128) == fa.FA_ERR_NULL_POINTER
    assert call(P, P, P, P, 1, 1, 1, 1 << 24, 1024, 64) == fa.FA_ERR_BAD_SHAPE
    assert call(P, P, P, P, 1024, 1024, 1024, 4096, 1024, 128) == fa.FA_ERR_BAD_SHAPE
    if paged:
        assert call(P, P, P, P, 1, 8, 2, 300, 1024, 128, table=None) == fa.FA_ERR_NULL_POINTER
        for psz in (0, 32, 96, -64, 1, 63, 65):
            assert call(P, P, P, P, 1, 8, 2, 300, 1024, 128, psz=psz, mpp=8) == fa.FA_ERR_BAD_SHAPE, psz
        for npages in (0, -1):
            assert call(P, P, P, P, 1, 8, 2, 300, 1024, 128, npages=npages) == fa.FA_ERR_BAD_SHAPE
        assert call(P, P, P, P, 1, 8, 2, 300, 1024, 128, mpp=-1) == fa.FA_ERR_BAD_SHAPE
        # logical capacity past INT_MAX - 64; the last one at or below it is accepted as a shape
        assert (INT_MAX - 64) // 64 * 64 == 2147483520
        assert call(P, P, P, P, 1, 8, 2, 300, 0, 128, psz=64, mpp=2147483520 // 64 + 1) == fa.FA_ERR_BAD_SHAPE
        assert call(None, P, P, P, 1, 8, 2, 300, 0, 128, psz=64, mpp=2147483520 // 64) == \
            fa.FA_ERR_NULL_POINTER
        # one page's rows of a head past a 32-bit byte range
        assert call(P, P, P, P, 1, 8, 2, 300, 0, 128, npages=1, psz=1 << 23, mpp=1) == fa.FA_ERR_BAD_SHAPE
    else:
        assert call(P, P, P, P, 1, 8, 2, 300, -5, 128) == fa.FA_ERR_BAD_SHAPE
        # a head's cache rows past a 32-bit byte range (the FP8 entries: the same capacities)
        assert call(P, P, P, P, 1, 8, 2, 300, 8388608, 128) == fa.FA_ERR_BAD_SHAPE
        assert call(P, P, P, P, 1, 8, 2, 300, 16777216, 64) == fa.FA_ERR_BAD_SHAPE
        assert call(None, P, P, P, 1, 8, 2, 300, 8388607, 128) == fa.FA_ERR_NULL_POINTER
    # empty problems: nothing to do, nothing launched, no pointer looked at
    assert call(None, None, None, None, 0, 8, 2, 300, 1024, 128, table=None) == fa.FA_OK
    assert call(None, None, None, None, 1, 0, 0, 300, 1024, 128, table=None) == fa.FA_OK
    if paged:  # ... but the page geometry is still checked
        assert call(None, None, None, None, 0, 8, 2, 300, 1024, 128, table=None, psz=96, mpp=8) == \
            fa.FA_ERR_BAD_SHAPE
    # rows but no keys: only o is needed (and missing here)
    assert call(None, None, None, None, 1, 8, 2, 300, 0, 128, table=None, mpp=0) == fa.FA_ERR_NULL_POINTER


def test_decode_entries_still_refuse_long_queries():
    """The prefill entries take over past 16 query tokens; decode's own bound stays."""
    lib = fa_mi355x.load_library()
    assert lib.fa_decode_f16(P, P, P, P, None, 1, 8, 2, 17, 1024, 128, None, 1, 0, None, 0, None) == \
        fa_mi355x.FA_ERR_BAD_SHAPE


# ---- the Python wrappers on CPU tensors: every rejection names its own cause --------

def _t(shape, dtype=torch.float16):
    return torch.zeros(shape, dtype=torch.float32).to(dtype)


def test_wrapper_rejections_contiguous():
    f = fa_mi355x.flash_attention_prefill
    q, k = _t((2, 4, 20, 64)), _t((2, 2, 128, 64))
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32)  # noqa: E731
    with pytest.raises(err, match="q must be float16 or bfloat16"):
        f(q.float(), k, k)
    with pytest.raises(err, match="k_cache and v_cache must have one dtype"):
        f(q, k.to(FP8), k)
    with pytest.raises(err, match=r"v_cache must be torch.float16, got torch.bfloat16"):
        f(q, k, k.to(torch.bfloat16))
    with pytest.raises(err, match="float8_e5m2 is not supported"):
        f(q, k.to(torch.float8_e5m2), k.to(torch.float8_e5m2))
    with pytest.raises(err, match=r"q must be 4-D \(BHSD\)"):
        f(q[0], k, k)
    with pytest.raises(err, match=r"k_cache must be 4-D \(BHSD\)"):
        f(q, k[0], k)
    with pytest.raises(err, match=r"out must be \[B,Hq,Sq,D\] like q"):
        f(q, k, k, out=_t((2, 4, 21, 64)))
    with pytest.raises(err, match="agree in batch and head_dim"):
        f(q, _t((3, 2, 128, 64)), _t((3, 2, 128, 64)))
    with pytest.raises(err, match="heads_q 4 is not a multiple of heads_kv 3"):
        f(q, _t((2, 3, 128, 64)), _t((2, 3, 128, 64)))
    with pytest.raises(err, match="q_lens must be int32, got torch.int64"):
        f(q, k, k, q_lens=torch.tensor([1, 2]))
    with pytest.raises(err, match=r"q_lens must be a contiguous \[B\] tensor"):
        f(q, k, k, q_lens=i32(1, 2, 3))
    with pytest.raises(err, match=r"q_lens must be a contiguous \[B\] tensor"):
        f(q, k, k, q_lens=i32(1, 2, 3, 4)[::2])
    with pytest.raises(err, match="kv_lens must be int32"):
        f(q, k, k, kv_lens=torch.tensor([1, 2]))
    with pytest.raises(err, match="go with a torch.float8_e4m3fn cache only"):
        f(q, k, k, k_scale=torch.ones(2))
    with pytest.raises(err, match=r"v_scale must be a contiguous float32 \[Hkv = 2\] tensor"):
        f(q, k.to(FP8), k.to(FP8), v_scale=torch.ones(3))
    # all shapes and dtypes in order: what is left is where the tensors live
    with pytest.raises(err, match="q must be a device tensor") as e:
        f(q, k, k, kv_lens=i32(5, 6), q_lens=i32(1, 2))
    assert e.value.status == fa_mi355x.FA_ERR_NULL_POINTER


def test_wrapper_rejections_paged():
    f = fa_mi355x.flash_attention_prefill_paged
    q, pool = _t((2, 4, 20, 64), torch.bfloat16), _t((5, 2, 128, 64), torch.bfloat16)
    table = torch.zeros((2, 3), dtype=torch.int32)
    with pytest.raises(err, match="block_table is required"):
        f(q, pool, pool, None)
    with pytest.raises(err, match="k_pages must be 4-D"):
        f(q, pool[0], pool, table)
    with pytest.raises(err, match="page_size 96 is not a positive multiple of 64"):
        f(q, _t((5, 2, 96, 64), torch.bfloat16), _t((5, 2, 96, 64), torch.bfloat16), table)
    with pytest.raises(err, match="block_table must be int32"):
        f(q, pool, pool, table.long())
    with pytest.raises(err, match="block_table has 3 rows, q a batch of 2"):
        f(q, pool, pool, torch.zeros((3, 3), dtype=torch.int32))
    with pytest.raises(err, match="q_lens must be int32, got torch.float32"):
        f(q, pool, pool, table, q_lens=torch.ones(2))
    with pytest.raises(err, match="go with a torch.float8_e4m3fn cache only"):
        f(q, pool, pool, table, v_scale=torch.ones(2))
    with pytest.raises(err, match="q must be a device tensor"):
        f(q, pool, pool, table, q_lens=torch.ones(2, dtype=torch.int32))


def test_torch_ops_registered_with_the_full_schema():
    import fa_mi355x.torch_op as top

    for op, lead in ((top.prefill, "Tensor q, Tensor k_cache, Tensor v_cache, "),
                     (top.prefill_paged, "Tensor q, Tensor k_pages, Tensor v_pages, Tensor block_table, ")):
        schema = str(op.default._schema)
        assert lead + ("Tensor? kv_lens=None, Tensor? q_lens=None, bool causal=True, Tensor? k_scale=None, "
                       "Tensor? v_scale=None) -> Tensor") in schema, schema
    q, k = _t((1, 2, 20, 64)), _t((1, 2, 64, 64))
    with pytest.raises(ValueError, match="needs GPU tensors"):
        top.prefill(q, k, k)
    with pytest.raises(ValueError, match="needs GPU tensors"):
        top.prefill_paged(q, k, k, torch.zeros((1, 1), dtype=torch.int32))
    from torch._subclasses.fake_tensor import FakeTensorMode

    with FakeTensorMode():
        fq = torch.empty((2, 8, 300, 128), dtype=torch.bfloat16)
        fk = torch.empty((2, 2, 512, 128), dtype=torch.bfloat16)
        assert top.prefill(fq, fk, fk).shape == fq.shape


# ---- compile-time resources ------------------------------------------------------------

UNITS = ["fa_prefill.hip", "fa_prefill_paged.hip", "fa_prefill_kv8.hip", "fa_prefill_paged_kv8.hip"]


def test_kernel_resource_usage():
    """No scratch in any prefill kernel, and no more LDS than the one constant
    csrc/fa_prefill_kernel.hpp documents (what the 4-wave loop of the forward
    kernel uses)."""
    src = open(os.path.join(cc.PKG, "csrc", "fa_prefill_kernel.hpp")).read()
    m = re.findall(r"constexpr int kPrefillLdsBytes = (\d+);", src)
    assert len(m) == 1, m
    lds_max = int(m[0])
    assert lds_max <= 4 * 64 * 256
    for unit, kernels in zip(UNITS, cc.kernel_resource_usage(UNITS)):
        mine = [x for x in kernels if "fa_prefill_kernel" in x[0]]
        assert len(mine) == 4, (unit, [x[0] for x in kernels])  # {fp16, bf16} x {128, 64}
        for name, scratch, lds in mine:
            print(f"{unit} {name}: scratch {scratch} LDS {lds}")
            assert scratch == 0, (unit, name, scratch)
            assert 0 < lds <= lds_max, (unit, name, lds)


# ---- the references against one another ------------------------------------------------

def _cpu(a):
    return torch.from_numpy(np.array(a, dtype=np.uint16).view(np.int16)).view(torch.float16)


# (B, Hq, Hkv, Sq, cap, D, q_lens, kv_lens): ragged chunks behind ragged prefixes;
# an element whose leading rows see nothing (kv_lens < n_b), one without rows
# and one without keys
REF_SHAPES = [
    (2, 4, 2, 40, 128, 64, (40, 23), (105, 23)),
    (3, 6, 2, 70, 192, 128, (70, 17, 0), (30, 192, 64)),
    (2, 2, 1, 33, 64, 64, (33, 20), (0, 64)),
]


@pytest.mark.parametrize("causal", [True, False], ids=["causal", "noncausal"])
@pytest.mark.parametrize("shape", REF_SHAPES, ids=lambda s: "x".join(map(str, s[:6])))
def test_references_agree(shape, causal):
    """oracle against fp32 torch against the float64 restatement of the
    contract, on the rows t < n_b: so the GPU tests do not rest on a reference
    that is wrong where decode's tests never looked (Sq > 16, q_lens)."""
    b, hq, hkv, sq, cap, d, q_lens, kv_lens = shape
    q, k, v = dr.inputs(b, hq, hkv, sq, cap, d)
    what = f"{shape} causal={causal}"
    o_oracle = pr.oracle_rows(q, k, v, kv_lens, q_lens, causal).view(np.float16).astype(np.float64)
    o_torch, lse_torch = pr.torch_rows(_cpu(q), _cpu(k), _cpu(v), kv_lens, q_lens, causal)
    lref, smax = pr.lse_rows(q, k, v, kv_lens, q_lens, causal)
    f64 = [a.view(np.float16).astype(np.float64) for a in (q, k, v)]
    o64, lse64, written = pr.contract_f64(*f64, kv_lens, q_lens, causal)
    vis = pr.visible(kv_lens, q_lens, b, sq, cap, causal)
    assert np.array_equal(written, vis >= 0), what
    for bi, n in enumerate(pr.n_rows(q_lens, b, sq)):
        assert not written[bi, n:].any() and written[bi, :n].all(), what
        if n == 0:
            continue
        unseen = vis[bi, :n] == 0
        # the float64 restatement is the judge: LSE of both others, then O
        assert np.array_equal(np.isneginf(lse64[bi, :, :n]), np.broadcast_to(unseen, (hq, n))), what
        dr.check_lse(torch.from_numpy(lref[bi, :, :n]), lse64[bi, :, :n], smax, what + " lse_ref")
        dr.check_lse(lse_torch[bi, :, :n], lse64[bi, :, :n], smax, what + " torch lse")
        ot = np.where(unseen[None, :, None], 0.0, o_torch[bi, :, :n].double().numpy())
        e_oracle = float(np.abs(o_oracle[bi, :, :n] - o64[bi, :, :n]).max())
        e_torch = float(np.abs(ot - o64[bi, :, :n]).max())
        print(f"{what} b={bi}: |oracle - f64| {e_oracle:.3e} |torch - f64| {e_torch:.3e}")
        assert e_oracle <= dr.GATE_F16 and e_torch <= dr.GATE_F16, (what, e_oracle, e_torch)
        assert not o_oracle[bi, :, :n][:, unseen].any() and not o64[bi, :, :n][:, unseen].any(), what


# ---- the key-sensitivity checkers on the float64 contract, at the GPU test's shapes ----

def _contract(q, k, v):
    o, lse, _ = pr.contract_f64(q.double().numpy(), k.double().numpy(), v.double().numpy(), pr.KS_KV_LENS,
                                pr.KS_Q_LENS, True)
    return torch.from_numpy(np.nan_to_num(o)), torch.from_numpy(np.nan_to_num(lse, nan=0.0))


@pytest.mark.parametrize("dtype", dr.DTYPES)
def test_census_checkers_accept_the_contract(dtype):
    """The census of tests/test_prefill_gpu.py on the float64 restatement
    rounded to the output type: the reference alone passes the checker."""
    assert ks.REL_GATE[dtype] <= ks.SIGNAL / 2
    for d, level, layout in ((128, 0.25, "tile"), (64, 0.0, "stripe")):
        q, k, v, counts = pr.ks_census(level, layout, d, dtype)
        o, lse = _contract(q, k, v)
        pr.ks_check_census(o.to(dtype).double(), lse, counts, level, layout,
                           f"census f64 {dr.name(dtype)} d={d} {level} {layout}", dtype=dtype)


@pytest.mark.parametrize("kind,d", [("diagonal", 128), ("sweep", 64)])
def test_needle_checkers_accept_the_contract(kind, d):
    q, k, v, pi, want = pr.ks_needle(kind, d, torch.float16)
    o, lse = _contract(q, k, v)
    pr.ks_check_needle(o, lse, q, k, pi, want, f"needle f64 {kind} d={d}")
    # the diagonal is the last visible key: off_b + t
    if kind == "diagonal":
        for bi, (n, ln) in enumerate(zip(pr.KS_Q_LENS, pr.KS_KV_LENS)):
            assert np.array_equal(pi[bi, 0, :n].numpy(), ln - n + np.arange(n))
    # one wrong key is seen: a census row that counts one key too many fails its checker
    q, k, v, counts = pr.ks_census(0.25, "stripe", d, torch.float16)
    o, lse = _contract(q, k, v)
    vis = pr.ks_visible(True)
    off_by_one = ks.check_census(o[0, :, :100].to(torch.float16).double(), vis[0, :, 1:101], counts, 0.25,
                                 "stripe", "off by one", dtype=torch.float16)
    assert not off_by_one.ok


# ---- the staircase inputs (prefill_refs.staircase) of tests/test_prefill_ranges_gpu.py --

ST_CASES = [(p, "q") for p in pr.ST_PATTERNS] + [(p, "scale") for p in ("asc4.5", "over8", "jump")]
ST_IDS = [f"{p}-{c}" for p, c in ST_CASES]
RESCALE_LOG2 = 8.0  # fa_fwd_kernel.hpp


@pytest.mark.parametrize("d", [128, 64])
@pytest.mark.parametrize("pattern,carry", [(p, c) for p in ("under8", "over8") for c in ("q", "scale")])
def test_staircase_steps_lie_on_the_intended_side_of_the_threshold(pattern, carry, d):
    """Clean patterns, float64: every visible row's maximum grows from one visible
    tile to the next by a step that is at least 0.05 log2 units below (under8) or
    above (over8) the kernel's rescale threshold, causal and not."""
    src = open(os.path.join(cc.PKG, "csrc", "fa_fwd_kernel.hpp")).read()
    assert re.findall(r"constexpr float RESCALE_LOG2 = ([0-9.]+)f;", src) == ["8.0"]
    st = pr.staircase(pattern, d, carry)
    assert not st.noisy
    kd = st.dequant()[0]
    g = pr.ST_HQ // pr.ST_HKV
    log2e_over_sqrt_d = math.log2(math.e) / math.sqrt(d)
    seen = 0
    for causal in (True, False):
        vis = pr.visible(pr.ST_KV_LENS, pr.ST_Q_LENS, pr.ST_B, pr.ST_SQ, pr.ST_CAP, causal)
        for bi in range(pr.ST_B):
            for h in range(pr.ST_HQ):
                s = st.q[bi, h] @ kd[bi, h // g].T * log2e_over_sqrt_d          # [Sq, cap], log2 units
                s = np.where(np.arange(pr.ST_CAP)[None, :] < vis[bi][:, None], s, -np.inf)
                tmax = s.reshape(pr.ST_SQ, -1, pr.ST_TILE).max(-1)              # [Sq, tiles]
                for t in range(pr.ST_Q_LENS[bi]):
                    row = tmax[t][np.isfinite(tmax[t])]
                    assert len(row) == -(-vis[bi, t] // pr.ST_TILE)
                    grow = np.diff(row)
                    seen += len(grow)
                    if pattern == "under8":
                        assert (grow > 4.0).all() and (grow <= RESCALE_LOG2 - 0.05).all(), (bi, h, t, grow)
                    else:
                        assert (grow >= RESCALE_LOG2 + 0.05).all(), (bi, h, t, grow)
    assert seen > 1000


@pytest.mark.parametrize("d", [128, 64])
@pytest.mark.parametrize("pattern,carry", ST_CASES, ids=ST_IDS)
def test_staircase_values_are_exact_in_every_type(pattern, carry, d):
    """Q in fp16 and bf16; what the cache holds in fp16, bf16 and E4M3 (and back);
    the scales in fp32, none of the carried ones a power of two."""
    st = pr.staircase(pattern, d, carry)
    for name, a, types in (("q", st.q, (torch.float16, torch.bfloat16)),
                           ("k", st.k, (torch.float16, torch.bfloat16, FP8)),
                           ("v", st.v, (torch.float16, torch.bfloat16, FP8))):
        t = torch.tensor(a)
        for ty in types:
            assert torch.equal(t.float().to(ty).double(), t), (name, ty)
    assert float(np.abs(st.v).max()) <= 0.5 and np.abs(st.levels).max() <= 8
    assert np.array_equal(st.k[..., 0], np.repeat(st.levels, pr.ST_TILE, axis=1)[:, None, :].repeat(pr.ST_HKV, 1))
    for s in (st.k_scale, st.v_scale):
        assert np.array_equal(s.astype(np.float32).astype(np.float64), s)
        if carry == "scale":
            assert (np.frexp(s)[0] != 0.5).all(), s
        else:
            assert (s == 1.0).all()
    if carry == "scale":
        assert (st.q[..., 0] == 1.0).all() and np.array_equal(st.k_scale, st.delta)
    else:
        assert np.array_equal(st.q[0, :, 0, 0], np.repeat(st.delta, pr.ST_HQ // pr.ST_HKV))
    if not st.noisy:
        assert not st.q[..., 1:].any()


@pytest.mark.parametrize("causal", [True, False], ids=["causal", "full"])
@pytest.mark.parametrize("d", [128, 64])
@pytest.mark.parametrize("dtype", dr.DTYPES)
@pytest.mark.parametrize("pattern,carry", ST_CASES, ids=ST_IDS)
def test_staircase_reference_alone_stays_inside_half_the_gates(pattern, carry, dtype, d, causal):
    """The model of the roundings the design allows (prefill_refs.st_model)
    against contract_f64 on the same inputs: at most HALF of each gate, for
    every pattern, dtype, head_dim and mask the GPU tests use."""
    st = pr.staircase(pattern, d, carry)
    o64, lse64, smax = pr.st_contract(pattern, d, carry, causal)
    om, lm = pr.st_model(st, dtype, pr.ST_KV_LENS, pr.ST_Q_LENS, causal)
    gate = dr.GATE_F16 if dtype is torch.float16 else dr.GATE_BF16
    lgate = 2.0 ** -10 * smax + 1e-5
    for bi, n in enumerate(pr.ST_Q_LENS):
        assert np.array_equal(np.isneginf(lm[bi, :, :n]), np.isneginf(lse64[bi, :, :n]))
        fin = np.isfinite(lse64[bi, :, :n])
        oerr = float(np.abs(om[bi, :, :n] - o64[bi, :, :n]).max())
        lerr = float(np.abs(lm[bi, :, :n][fin] - lse64[bi, :, :n][fin]).max())
        print(f"{pattern} {carry} {dr.name(dtype)} d={d} causal={causal} b={bi}: O {oerr:.3e} of {gate:.0e}, "
              f"LSE {lerr:.3e} of {lgate:.3e}")
        assert oerr <= gate / 2, (bi, oerr)
        assert lerr <= lgate / 2, (bi, lerr, lgate)


@pytest.mark.parametrize("causal", [True, False], ids=["causal", "full"])
@pytest.mark.parametrize("d", [128, 64])
@pytest.mark.parametrize("pattern", list(pr.ST_PATTERNS))
def test_staircase_oracle_agrees_with_the_contract(pattern, d, causal):
    """fp16 on a 16-bit cache is judged by the CPU oracle: on these inputs it and
    contract_f64 agree within half the gate."""
    st = pr.staircase(pattern, d, "q")
    host = tuple(dr.bits(torch.tensor(a).to(torch.float16)) for a in (st.q, st.k, st.v))
    oo = pr.oracle_rows(*host, pr.ST_KV_LENS, pr.ST_Q_LENS, causal).view(np.float16).astype(np.float64)
    o64 = pr.st_contract(pattern, d, "q", causal)[0]
    for bi, n in enumerate(pr.ST_Q_LENS):
        err = float(np.abs(oo[bi, :, :n] - o64[bi, :, :n]).max())
        print(f"{pattern} d={d} causal={causal} b={bi}: |oracle - f64| {err:.3e}")
        assert err <= dr.GATE_F16 / 2, (bi, err)
