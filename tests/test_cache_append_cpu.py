"""CPU tests of the cache-append entries (fa_cache_append_16 / _paged_16 /
_kv8_f16 / _kv8_bf16 / _paged_kv8_f16 / _paged_kv8_bf16,
fa_mi355x.flash_attention_cache_append[_paged] and the torch ops): exports,
the argument checks with fake pointers, the wrappers' rejections, the ops'
schemas and fake implementations, the FP8 contract pinned by an integer-only
reference against torch's CPU conversion over every 16-bit pattern, and the
kernels' compile-time resource usage -- no kernel is launched (no GPU here)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import capi_checks
from capi_checks import fa as _fa
from fp8_contract import NAN_PATTERNS, all_patterns, integer_reference_bytes, torch_reference_bytes

SYMBOLS = ("fa_cache_append_16", "fa_cache_append_paged_16", "fa_cache_append_kv8_f16",
           "fa_cache_append_kv8_bf16", "fa_cache_append_paged_kv8_f16",
           "fa_cache_append_paged_kv8_bf16")
FP8 = torch.float8_e4m3fn
SCALES = (1.0, 2.0 ** -6, 0.3, 3.7)


# ---------------------------------------------------------------------------
# The contract of the FP8 cache (tests/fp8_contract.py): the torch expression
# on the CPU against the integer-only model of it.

@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
def test_fp8_contract_integer_model_equals_torch_cpu(dtype):
    x = all_patterns(dtype)
    bits = x.view(torch.int16).numpy().view(np.uint16)
    for s in SCALES:
        want = torch_reference_bytes(x, s).numpy()
        got, is_nan = integer_reference_bytes(bits, dtype, s)
        assert int(is_nan.sum()) == NAN_PATTERNS[dtype]
        assert np.array_equal(is_nan, torch.isnan(x.float()).numpy())
        bad = np.flatnonzero((got != want) & ~is_nan)
        assert bad.size == 0, (s, [(hex(bits[i]), hex(got[i]), hex(want[i])) for i in bad[:8]])
        assert np.all((want[is_nan] & 0x7f) == 0x7f) and np.all((got[is_nan] & 0x7f) == 0x7f)


def test_fp8_contract_landmarks():
    """The cases the contract names, through the integer model."""
    def one(value, scale=1.0, dtype=torch.float16):
        bits = torch.tensor([value], dtype=dtype).view(torch.int16).numpy().view(np.uint16)
        return int(integer_reference_bytes(bits, dtype, scale)[0][0])

    assert one(float("inf")) == 0x7e and one(float("-inf")) == 0xfe   # saturate
    assert one(1000.0) == 0x7e and one(464.0) == 0x7e and one(-60000.0) == 0xfe
    assert one(0.0) == 0x00 and one(-0.0) == 0x80                      # the zero's sign
    assert one(2.0 ** -9) == 0x01 and one(2.0 ** -10) == 0x00          # tie to even: 0
    assert one(3 * 2.0 ** -10) == 0x02 and one(-(2.0 ** -11)) == 0x80  # tie to even: 2
    assert one(2.0 ** -6) == 0x08 and one(1.0) == 0x38
    assert one(1.0, 2.0 ** -6) == 0x68                                 # 64
    assert one(1.0, 0.3, torch.bfloat16) == 0x45                       # 3.333 -> 3.25


# ---------------------------------------------------------------------------
# Exports and argument checks

def test_library_exports_append_symbols():
    capi_checks.assert_exported(SYMBOLS)


P = ctypes.c_void_p


def _call(name, **kw):
    """One entry with fake pointers; keyword arguments override the defaults."""
    a = dict(k_new=P(0x1000), v_new=P(0x2000), k_cache=P(0x3000), v_cache=P(0x4000), batch=2,
             heads_kv=2, seqlen_new=3, kv_capacity=256, head_dim=128, num_pages=8, page_size=64,
             block_table=P(0x5000), max_pages_per_seq=4, kv_lens=P(0x6000), new_lens=None, stream=None,
             k_scale=None, v_scale=P(0x7000))
    unknown = set(kw) - set(a)
    assert not unknown, unknown
    a.update(kw)
    args = [a["k_new"], a["v_new"], a["k_cache"], a["v_cache"], a["batch"], a["heads_kv"],
            a["seqlen_new"]]
    if "paged" in name:
        args += [a["head_dim"], a["num_pages"], a["page_size"], a["block_table"],
                 a["max_pages_per_seq"]]
    else:
        args += [a["kv_capacity"], a["head_dim"]]
    args += [a["kv_lens"], a["new_lens"], a["stream"]]
    if "kv8" in name:
        args += [a["k_scale"], a["v_scale"]]
    return getattr(_fa().load_library(), name)(*args)


@pytest.mark.parametrize("name", SYMBOLS)
def test_argument_checks(name):
    """Every status of the header, each returned before any HIP call (the
    pointers are fake and there is no GPU here)."""
    fa = _fa()
    paged = "paged" in name
    bad, dim, null, ok = (fa.FA_ERR_BAD_SHAPE, fa.FA_ERR_UNSUPPORTED_HEAD_DIM, fa.FA_ERR_NULL_POINTER,
                          fa.FA_OK)
    # negative sizes, before the head_dim check
    assert _call(name, batch=-1) == bad
    assert _call(name, heads_kv=-1, head_dim=96) == bad
    assert _call(name, head_dim=-128) == bad
    if not paged:
        assert _call(name, kv_capacity=-1) == bad
    for d in (0, 32, 96, 256):
        assert _call(name, head_dim=d) == dim
    assert _call(name, head_dim=96, seqlen_new=0) == dim       # head_dim before seqlen_new
    for sn in (0, -1, 0x7fffffff - 63):
        assert _call(name, seqlen_new=sn) == bad
    assert _call(name, seqlen_new=0, batch=0) == bad            # shape errors before emptiness
    if paged:
        for ps in (0, -64, 32, 96, 65):
            assert _call(name, page_size=ps) == bad
        assert _call(name, num_pages=0) == bad
        assert _call(name, num_pages=-1) == bad
        assert _call(name, max_pages_per_seq=-1) == bad
        assert _call(name, page_size=1 << 23) == bad            # page_size * 2 * head_dim > INT_MAX
        assert _call(name, page_size=1 << 24, head_dim=64) == bad
        assert _call(name, page_size=64, max_pages_per_seq=1 << 25) == bad   # capacity > INT_MAX - 64
        assert _call(name, page_size=0, batch=0) == bad
        assert _call(name, block_table=None) == null
        assert _call(name, max_pages_per_seq=0, block_table=None, kv_lens=None) == ok   # capacity 0
    else:
        assert _call(name, kv_capacity=1 << 23) == bad          # cap * 2 * head_dim > INT_MAX
        assert _call(name, kv_capacity=1 << 24, head_dim=64) == bad
        assert _call(name, kv_capacity=1 << 23, batch=0) == ok  # emptiness before the range
        assert _call(name, kv_capacity=0, k_cache=None, kv_lens=None) == ok
    # empty problems: FA_OK with nothing enqueued, whatever the pointers
    assert _call(name, batch=0, k_new=None, kv_lens=None) == ok
    assert _call(name, heads_kv=0, v_cache=None) == ok
    for ptr in ("k_new", "v_new", "k_cache", "v_cache", "kv_lens"):
        assert _call(name, **{ptr: None}) == null, ptr


# ---------------------------------------------------------------------------
# Wrappers and ops (meta tensors)

def _t(shape, dtype=torch.float16, device="meta"):
    return torch.empty(shape, dtype=dtype, device=device)


def test_python_wrapper_rejections():
    """One rejection per cause, each raised before the device is looked at;
    an accepted call gets as far as the device check."""
    fa = _fa()
    N, C, PG = (2, 2, 3, 128), (2, 2, 256, 128), (8, 2, 64, 128)
    i32, f32 = torch.int32, torch.float32
    lens, tab, sc = _t((2,), i32), _t((2, 4), i32), _t((2,), f32)

    def both(match, k_new=None, v_new=None, kc=None, vc=None, kp=None, vp=None, table=tab, kv_lens=lens,
             which=("c", "p"), **kw):
        k_new = _t(N) if k_new is None else k_new
        v_new = _t(N) if v_new is None else v_new
        if "c" in which:
            with pytest.raises(fa.FlashAttentionError, match=match):
                fa.flash_attention_cache_append(k_new, v_new, _t(C) if kc is None else kc,
                                                _t(C) if vc is None else vc, kv_lens, **kw)
        if "p" in which:
            with pytest.raises(fa.FlashAttentionError, match=match):
                fa.flash_attention_cache_append_paged(k_new, v_new, _t(PG) if kp is None else kp,
                                                      _t(PG) if vp is None else vp, table, kv_lens, **kw)

    both("k_new must be float16 or bfloat16", k_new=_t(N, f32))
    both("v_new must be torch.float16, got torch.bfloat16", v_new=_t(N, torch.bfloat16))
    both("must have one dtype, got torch.float8_e4m3fn and torch.float16", kc=_t(C, FP8), kp=_t(PG, FP8))
    both("torch.float8_e5m2 is not supported", kc=_t(C, torch.float8_e5m2), vc=_t(C, torch.float8_e5m2),
         kp=_t(PG, torch.float8_e5m2), vp=_t(PG, torch.float8_e5m2))
    both("(k_cache|k_pages) must be torch.float16, got torch.bfloat16", kc=_t(C, torch.bfloat16),
         kp=_t(PG, torch.bfloat16))
    both("go with a torch.float8_e4m3fn cache only", k_scale=sc)
    both("k_new must be 4-D", k_new=_t((2, 2, 128)), v_new=_t((2, 2, 128)))
    both("v_new must be contiguous", v_new=_t((2, 2, 6, 128))[:, :, ::2])
    both("v_cache must be contiguous", vc=_t((2, 2, 512, 128))[:, :, ::2], which="c")   # a strided cache
    both("k_new and v_new must have one shape", v_new=_t((2, 2, 4, 128)))
    both("k_new holds no token", k_new=_t((2, 2, 0, 128)), v_new=_t((2, 2, 0, 128)))
    both("(k_cache and v_cache|k_pages and v_pages) must have one shape", vc=_t((2, 2, 128, 128)),
         vp=_t((9, 2, 64, 128)))
    both("must agree in heads_kv and head_dim", kc=_t((2, 4, 256, 128)), vc=_t((2, 4, 256, 128)),
         kp=_t((8, 4, 64, 128)), vp=_t((8, 4, 64, 128)))
    both("must agree in heads_kv and head_dim", kc=_t((2, 2, 256, 64)), vc=_t((2, 2, 256, 64)),
         kp=_t((8, 2, 64, 64)), vp=_t((8, 2, 64, 64)))
    both("k_new and the caches must agree in batch", kc=_t((3, 2, 256, 128)), vc=_t((3, 2, 256, 128)),
         which="c")
    both("the page pools hold no page", kp=_t((0, 2, 64, 128)), vp=_t((0, 2, 64, 128)), which="p")
    both("page_size 96 is not a positive multiple of 64", kp=_t((8, 2, 96, 128)), vp=_t((8, 2, 96, 128)),
         which="p")
    both("kv_lens is required", kv_lens=None)
    both("new_lens must be int32", new_lens=_t((2,), torch.int64))
    both("new_lens must be a contiguous \\[B\\] tensor", new_lens=_t((3,), i32))
    both("v_scale must be a contiguous float32 \\[Hkv = 2\\] tensor", kc=_t(C, FP8), vc=_t(C, FP8),
         kp=_t(PG, FP8), vp=_t(PG, FP8), v_scale=_t((3,), f32))
    both("block_table must be int32", table=_t((2, 4), torch.int64), which="p")
    both("block_table has 3 rows, k_new a batch of 2", table=_t((3, 4), i32), which="p")
    both("block_table is required", table=None, which="p")
    both("kv_lens must be int32", kv_lens=_t((2,), torch.int64))
    both("kv_lens must be a contiguous \\[B\\] tensor", kv_lens=_t((3,), i32))
    # nothing wrong but the device: 16-bit and FP8 calls were accepted
    both("k_new must be a device tensor")
    both("k_new must be a device tensor", new_lens=lens)
    both("k_new must be a device tensor", k_new=_t(N, torch.bfloat16), v_new=_t(N, torch.bfloat16),
         kc=_t(C, FP8), vc=_t(C, FP8), kp=_t(PG, FP8), vp=_t(PG, FP8), k_scale=sc, v_scale=sc)


def test_ops_schemas_fake_and_cpu():
    import fa_mi355x.torch_op as top  # noqa: F401

    assert str(torch.ops.fa_mi355x.cache_append.default._schema) == (
        "fa_mi355x::cache_append(Tensor k_new, Tensor v_new, Tensor(a!) k_cache, Tensor(b!) v_cache, "
        "Tensor kv_lens, Tensor? new_lens=None, Tensor? k_scale=None, Tensor? v_scale=None) -> ()")
    assert str(torch.ops.fa_mi355x.cache_append_paged.default._schema) == (
        "fa_mi355x::cache_append_paged(Tensor k_new, Tensor v_new, Tensor(a!) k_pages, "
        "Tensor(b!) v_pages, Tensor block_table, Tensor kv_lens, Tensor? new_lens=None, "
        "Tensor? k_scale=None, Tensor? v_scale=None) -> ()")
    lens, tab, sc = _t((2,), torch.int32), _t((2, 4), torch.int32), _t((2,), torch.float32)
    for dtype in (torch.float16, torch.bfloat16):
        for cdt in (dtype, FP8):
            n, c, pg = _t((2, 2, 3, 128), dtype), _t((2, 2, 256, 128), cdt), _t((8, 2, 64, 128), cdt)
            scales = (sc, sc) if cdt is FP8 else (None, None)
            assert torch.ops.fa_mi355x.cache_append(n, n, c, c, lens) is None
            assert torch.ops.fa_mi355x.cache_append(n, n, c, c, lens, lens, *scales) is None
            assert torch.ops.fa_mi355x.cache_append_paged(n, n, pg, pg, tab, lens) is None
            assert torch.ops.fa_mi355x.cache_append_paged(n, n, pg, pg, tab, lens, lens, *scales) is None
    n = torch.zeros((1, 2, 1, 128), dtype=torch.float16)
    c = torch.zeros((1, 2, 64, 128), dtype=torch.float16)
    one = torch.ones(1, dtype=torch.int32)
    with pytest.raises(ValueError):  # no CPU path
        torch.ops.fa_mi355x.cache_append(n, n, c, c, one)
    with pytest.raises(ValueError):
        torch.ops.fa_mi355x.cache_append_paged(n, n, c, c, torch.zeros((1, 1), dtype=torch.int32), one)
    assert not c.any()


# ---------------------------------------------------------------------------
# Compile-time resource usage

@pytest.mark.skipif(not os.path.exists(capi_checks.HIPCC), reason="needs hipcc")
def test_append_kernels_use_no_scratch_and_no_lds():
    """16-bit: 2 head dims x contiguous / paged = 4 kernels (one bit copy for
    fp16 and bf16); FP8: 2 source types x 2 head dims x contiguous / paged = 8.
    Every one compiles for gfx950 with no scratch and no LDS."""
    (kernels,) = capi_checks.kernel_resource_usage(["fa_cache_append.hip"], timeout=900)
    names, scratch, lds = (list(x) for x in zip(*kernels))
    assert len(names) == 12, (names, scratch, lds)
    assert len(set(names)) == 12 and all("fa_cache_append_kernel" in n for n in names), names
    assert sum("Lb1EEEvNS" in n for n in names) == 8, names     # KV8 = true
    assert not any(scratch), dict(zip(names, scratch))
    assert not any(lds), dict(zip(names, lds))
