"""CPU tests of the fused RoPE + cache-append entries (fa_rope_append_* and
fa_rope_append_varlen_*, fa_mi355x.flash_attention_rope_append[_varlen][_paged]
and the torch ops): exports, the argument checks with fake pointers, the
wrappers' rejections, the ops' schemas and fake implementations, the kernels'
compile-time resource usage, and the references of tests/rope_refs.py against
a float64 restatement -- no kernel is launched (no GPU here)."""
import ctypes
import os

import pytest
import torch

import capi_checks
import rope_refs
from capi_checks import fa as _fa

FORMS = ("", "_paged", "_kv8", "_paged_kv8")
SYMBOLS = tuple("fa_rope_append" + fam + form + ty for fam in ("", "_varlen") for form in FORMS
                for ty in ("_f16", "_bf16"))
FP8 = torch.float8_e4m3fn
# the append tests' cases: per Sn, the lengths AFTER the append
LENS = {1: (1, 0, 192), 3: (65, 2, 197), 16: (70, 16, 192), 67: (67, 197, 30)}


def test_library_exports_rope_append_symbols():
    assert len(SYMBOLS) == 16
    capi_checks.assert_exported(SYMBOLS)


P = ctypes.c_void_p


def _call(name, **kw):
    """One entry with fake pointers; keyword arguments override the defaults."""
    a = dict(k_new=P(0x1000), v_new=P(0x2000), k_cache=P(0x3000), v_cache=P(0x4000), batch=2,
             heads_kv=2, seqlen_new=3, kv_capacity=256, head_dim=128, num_pages=8, page_size=64,
             block_table=P(0x5000), max_pages_per_seq=4, kv_lens=P(0x6000), new_lens=P(0x6100), stream=None,
             k_scale=None, v_scale=P(0x7000), q=P(0x8000), q_out=P(0x9000), heads_q=4, cos=P(0xa000),
             sin=P(0xb000), rope_len=512, rotary_dim=64, interleaved=0)
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
    args += [a["q"], a["q_out"], a["heads_q"], a["cos"], a["sin"], a["rope_len"], a["rotary_dim"],
             a["interleaved"]]
    return getattr(_fa().load_library(), name)(*args)


@pytest.mark.parametrize("name", SYMBOLS)
def test_argument_checks(name):
    """Every status of the header, each returned before any HIP call (the
    pointers are fake and there is no GPU here): the append's own in the
    append's order (tests/test_cache_append_cpu.py), the rotary ones among them."""
    fa = _fa()
    paged, varlen = "paged" in name, "varlen" in name
    bad, dim, null, ok = (fa.FA_ERR_BAD_SHAPE, fa.FA_ERR_UNSUPPORTED_HEAD_DIM, fa.FA_ERR_NULL_POINTER,
                          fa.FA_OK)
    # ---- the append's
    assert _call(name, batch=-1) == bad
    assert _call(name, heads_kv=-1, head_dim=96) == bad
    assert _call(name, head_dim=-128) == bad
    if not paged:
        assert _call(name, kv_capacity=-1) == bad
    for d in (0, 32, 96, 256):
        assert _call(name, head_dim=d) == dim
    assert _call(name, head_dim=96, seqlen_new=-1) == dim      # head_dim before seqlen_new
    for sn in (-1, 0x7fffffff - 63) + (() if varlen else (0,)):
        assert _call(name, seqlen_new=sn) == bad
    assert _call(name, seqlen_new=-1, batch=0) == bad           # shape errors before emptiness
    if varlen:
        assert _call(name, seqlen_new=0, k_new=None, cos=None) == ok    # no token: nothing enqueued
        assert _call(name, new_lens=None) == null               # cu_seqlens is required
        # the grid: total_new / TB + batch past INT_MAX
        assert _call(name, seqlen_new=0x7fffffff - 64, batch=0x7fffffff - 100, head_dim=64) == bad
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
        # capacity 0: no K/V row; nothing at all without query heads, else Q alone
        assert _call(name, max_pages_per_seq=0, block_table=None, kv_lens=None, heads_q=0, q=None,
                     q_out=None, cos=None) == ok
        assert _call(name, max_pages_per_seq=0, block_table=None, k_new=None, q=None) == null
    else:
        assert _call(name, kv_capacity=1 << 23) == bad          # cap * 2 * head_dim > INT_MAX
        assert _call(name, kv_capacity=1 << 24, head_dim=64) == bad
        assert _call(name, kv_capacity=1 << 23, batch=0) == ok  # emptiness before the range
        assert _call(name, kv_capacity=0, k_cache=None, kv_lens=None, heads_q=0, q=None, q_out=None,
                     cos=None) == ok
        assert _call(name, kv_capacity=0, k_cache=None, k_new=None, q=None) == null
    assert _call(name, batch=0, k_new=None, kv_lens=None, cos=None) == ok
    assert _call(name, heads_kv=0, heads_q=0, v_cache=None, q=None, sin=None) == ok
    for ptr in ("k_new", "v_new", "k_cache", "v_cache", "kv_lens"):
        assert _call(name, **{ptr: None}) == null, ptr
    # ---- the rotary ones
    assert _call(name, heads_q=-1) == bad
    assert _call(name, heads_q=-1, head_dim=96) == bad          # with the negative sizes
    for r in (0, -16, 8, 24, 100, 144, 256):
        assert _call(name, rotary_dim=r) == bad, r
    assert _call(name, rotary_dim=128, head_dim=64) == bad      # R <= head_dim
    assert _call(name, rotary_dim=96, head_dim=64) == bad
    for r in (16, 32, 96, 128):                                  # accepted as a shape: fails later
        assert _call(name, rotary_dim=r, cos=None) == null, r
    assert _call(name, rotary_dim=24, head_dim=96) == dim       # head_dim before rotary_dim
    for n in (0, -1):
        assert _call(name, rope_len=n) == bad
    assert _call(name, rope_len=0, cos=None) == bad             # shapes before pointers
    assert _call(name, rotary_dim=8, batch=0) == bad            # ... and before emptiness
    assert _call(name, cos=None) == null
    assert _call(name, sin=None) == null
    assert _call(name, q=None) == null
    assert _call(name, q_out=None) == null
    assert _call(name, k_new=None, cos=P(0xa004)) == null       # pointers before the alignment
    assert _call(name, cos=P(0xa004)) == bad                    # 16-byte aligned tables
    assert _call(name, sin=P(0xb008)) == bad


def _t(shape, dtype=torch.float16, device="meta"):
    return torch.empty(shape, dtype=dtype, device=device)


def test_python_wrapper_rejections():
    """One rejection per rotary cause, each raised before the device is looked
    at; the append's own rejections follow them, and an accepted call gets as
    far as the device check."""
    fa = _fa()
    i32, f32 = torch.int32, torch.float32
    lens, tab, cu = _t((2,), i32), _t((2, 4), i32), _t((3,), i32)
    C, PG = (2, 2, 256, 128), (8, 2, 64, 128)

    def all4(match, q="default", k_new=None, cos=None, sin=None, which="cpvw", **kw):
        """c / p: padded contiguous / paged; v / w: packed contiguous / paged."""
        cos = _t((512, 32), f32) if cos is None else cos
        sin = _t((512, 32), f32) if sin is None else sin
        for w in which:
            packed, paged = w in "vw", w in "pw"
            kn = k_new if k_new is not None else _t((7, 2, 128) if packed else (2, 2, 3, 128))
            qq = q if not isinstance(q, str) else _t((7, 4, 128) if packed else (2, 4, 3, 128))
            if isinstance(qq, dict):
                qq = qq[packed]
            caches = (_t(PG), _t(PG), tab) if paged else (_t(C), _t(C))
            fn = getattr(fa, "flash_attention_rope_append" + ("_varlen" if packed else "")
                         + ("_paged" if paged else ""))
            args = (qq, kn, kn, *caches, *((cu, lens) if packed else (lens,)), cos, sin)
            with pytest.raises(fa.FlashAttentionError, match=match):
                fn(*args, **kw)

    all4("cos must be float32", cos=_t((512, 32), torch.float16))
    all4("sin must be float32", sin=_t((512, 32), torch.float64))
    all4("cos must be a contiguous \\[rope_len, R/2\\] tensor", cos=_t((512, 64), f32)[:, ::2])
    all4("sin must be a contiguous \\[rope_len, R/2\\] tensor", sin=_t((512,), f32))
    all4("cos and sin must have one shape", sin=_t((512, 16), f32))
    all4("rope_len must be >= 1", cos=_t((0, 32), f32), sin=_t((0, 32), f32))
    all4("rotary_dim 24 ", cos=_t((512, 12), f32), sin=_t((512, 12), f32))
    all4("rotary_dim 256 ", cos=_t((512, 128), f32), sin=_t((512, 128), f32))
    all4("rotary_dim 0 ", cos=_t((512, 0), f32), sin=_t((512, 0), f32))
    all4("cos is required", cos=3.0)
    all4("q_out goes with q only", q=None, q_out=_t((2, 4, 3, 128)))
    all4("q must be torch.float16 like k_new", q={False: _t((2, 4, 3, 128), torch.bfloat16),
                                                   True: _t((7, 4, 128), torch.bfloat16)})
    all4("q must be a contiguous \\[B,Hq,Sn,D\\] tensor", q=_t((2, 4, 6, 128))[:, :, ::2], which="cp")
    all4("q must be a contiguous \\[T,Hq,D\\] tensor", q=_t((2, 4, 3, 128)), which="vw")
    all4("q must be \\[B,Hq,Sn,D\\] with k_new's extents but for the heads", q=_t((2, 4, 4, 128)), which="cp")
    all4("q must be \\[B,Hq,Sn,D\\] with k_new's extents but for the heads", q=_t((2, 4, 3, 64)), which="cp")
    all4("q must be \\[T,Hq,D\\] with k_new's extents but for the heads", q=_t((8, 4, 128)), which="vw")
    all4("q_out must have q's shape", q_out=_t((2, 5, 3, 128)), which="cp")
    all4("q_out must be torch.float16 like k_new", q_out=_t((2, 4, 3, 128), torch.bfloat16), which="cp")
    # the append's own rejections follow
    all4("k_new must be float16 or bfloat16", k_new=_t((2, 2, 3, 128), f32), q=None, which="cp")
    # nothing wrong but the device: accepted with and without q, in place, both styles
    all4("k_new must be a device tensor")
    all4("k_new must be a device tensor", q=None)
    all4("k_new must be a device tensor", interleaved=True)
    q = _t((2, 4, 3, 128))
    all4("k_new must be a device tensor", q=q, q_out=q, which="cp")
    all4("k_new must be a device tensor", cos=_t((512, 64), f32), sin=_t((512, 64), f32))   # R = D


def test_ops_schemas_fake_and_cpu():
    import fa_mi355x.torch_op as top  # noqa: F401

    ops = torch.ops.fa_mi355x
    tail = ("Tensor cos, Tensor sin, {}bool interleaved=False, Tensor? k_scale=None, "
            "Tensor? v_scale=None) -> Tensor")
    assert str(ops.rope_append.default._schema) == (
        "fa_mi355x::rope_append(Tensor q, Tensor k_new, Tensor v_new, Tensor(a!) k_cache, "
        "Tensor(b!) v_cache, Tensor kv_lens, " + tail.format("Tensor? new_lens=None, "))
    assert str(ops.rope_append_paged.default._schema) == (
        "fa_mi355x::rope_append_paged(Tensor q, Tensor k_new, Tensor v_new, Tensor(a!) k_pages, "
        "Tensor(b!) v_pages, Tensor block_table, Tensor kv_lens, " + tail.format("Tensor? new_lens=None, "))
    assert str(ops.rope_append_varlen.default._schema) == (
        "fa_mi355x::rope_append_varlen(Tensor q, Tensor k_new, Tensor v_new, Tensor(a!) k_cache, "
        "Tensor(b!) v_cache, Tensor cu_seqlens, Tensor kv_lens, " + tail.format(""))
    assert str(ops.rope_append_varlen_paged.default._schema) == (
        "fa_mi355x::rope_append_varlen_paged(Tensor q, Tensor k_new, Tensor v_new, Tensor(a!) k_pages, "
        "Tensor(b!) v_pages, Tensor block_table, Tensor cu_seqlens, Tensor kv_lens, " + tail.format(""))
    i32, f32 = torch.int32, torch.float32
    lens, tab, cu, sc = _t((2,), i32), _t((2, 4), i32), _t((3,), i32), _t((2,), f32)
    cos = _t((512, 32), f32)
    for dtype in (torch.float16, torch.bfloat16):
        for cdt in (dtype, FP8):
            q, n = _t((2, 4, 3, 128), dtype), _t((2, 2, 3, 128), dtype)
            qp, npk = _t((7, 4, 128), dtype), _t((7, 2, 128), dtype)
            c, pg = _t((2, 2, 256, 128), cdt), _t((8, 2, 64, 128), cdt)
            kw = dict(k_scale=sc, v_scale=sc) if cdt is FP8 else {}
            for out, like in ((ops.rope_append(q, n, n, c, c, lens, cos, cos, **kw), q),
                              (ops.rope_append(q, n, n, c, c, lens, cos, cos, lens, True, **kw), q),
                              (ops.rope_append_paged(q, n, n, pg, pg, tab, lens, cos, cos, **kw), q),
                              (ops.rope_append_varlen(qp, npk, npk, c, c, cu, lens, cos, cos, **kw), qp),
                              (ops.rope_append_varlen_paged(qp, npk, npk, pg, pg, tab, cu, lens, cos, cos,
                                                            interleaved=True, **kw), qp)):
                assert out.shape == like.shape and out.dtype == like.dtype and out.device == like.device
    q = torch.zeros((1, 4, 1, 128), dtype=torch.float16)
    n = torch.zeros((1, 2, 1, 128), dtype=torch.float16)
    c = torch.zeros((1, 2, 64, 128), dtype=torch.float16)
    one, cs = torch.ones(1, dtype=i32), torch.zeros((8, 64))
    with pytest.raises(ValueError):  # no CPU path
        ops.rope_append(q, n, n, c, c, one, cs, cs)
    with pytest.raises(ValueError):
        ops.rope_append_paged(q, n, n, c, c, torch.zeros((1, 1), dtype=i32), one, cs, cs)
    with pytest.raises(ValueError):
        ops.rope_append_varlen(q[0], n[0], n[0], c, c, torch.zeros(2, dtype=i32), one, cs, cs)
    assert not c.any()


@pytest.mark.skipif(not os.path.exists(capi_checks.HIPCC), reason="needs hipcc")
def test_rope_append_kernels_use_no_scratch_and_no_lds():
    """Per unit 2 types x 2 head dims x contiguous / paged x 16-bit / FP8 = 16
    kernels (R and the pair style are launch parameters, not instantiations).
    Every one compiles for gfx950 with no scratch and no LDS."""
    units = ["fa_rope_append.hip", "fa_rope_append_varlen.hip"]
    for unit, kernels in zip(units, capi_checks.kernel_resource_usage(units, timeout=900)):
        names, scratch, lds = (list(x) for x in zip(*kernels))
        assert len(names) == 16, (unit, names)
        assert len(set(names)) == 16 and all("fa_rope_append_kernel" in n for n in names), names
        assert sum("PackedSrc" in n for n in names) == (16 if "varlen" in unit else 0), names
        assert not any(scratch), dict(zip(names, scratch))
        assert not any(lds), dict(zip(names, lds))


# ---------------------------------------------------------------------------
# The references (tests/rope_refs.py)

def _inputs(dtype, shape, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=g).to(dtype)
    flat = x.view(-1)
    flat[::97] = 0.0
    flat[5::193] = -0.0
    return x


@pytest.mark.parametrize("interleaved", [False, True], ids=["neox", "gptj"])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
def test_reference_against_float64(dtype, interleaved):
    """The contract's fp32 expression against float64: within one 16-bit ulp
    everywhere and equal on at least 99 % of the elements of these inputs."""
    r, d = 96, 128
    cos, sin = rope_refs.rope_tables(256, r)
    x = _inputs(dtype, (3, 2, 67, d), 1)
    lens = LENS[67]
    got, valid = rope_refs.rotate_tokens(x, cos, sin, lens, None, interleaved)
    pos, _ = rope_refs.positions(lens, 67)
    p = pos.clamp(0, 255)
    want = torch.where(valid[:, None, :, None],
                       rope_refs.rotate_f64(x, cos[p][:, None], sin[p][:, None], interleaved), x)
    dist = (rope_refs.ordered(got) - rope_refs.ordered(want)).abs()
    assert int(dist.max()) <= 1
    share = float((dist == 0).float().mean())
    assert share >= 0.99, share
    assert bool(valid.any()) and not bool(valid.all())
    assert not torch.equal(got.view(torch.int16), x.view(torch.int16))  # something was rotated


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
def test_style_identity(dtype):
    """Interleaved rotation of x == un-permuting the NeoX rotation of the permuted x, bit for bit."""
    r, d = 32, 64
    cos, sin = rope_refs.rope_tables(64, r)
    x = _inputs(dtype, (2, 3, 16, d), 2)
    c, s = cos[5:21][None, None], sin[5:21][None, None]
    perm = torch.cat([torch.arange(0, r, 2), torch.arange(1, r, 2), torch.arange(r, d)])  # neox <- gptj
    inv = torch.argsort(perm)
    a = rope_refs.rotate(x, c, s, True)
    b = rope_refs.rotate(x[..., perm], c, s, False)[..., inv]
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))
    assert not torch.equal(a.view(torch.int16), x.view(torch.int16))


@pytest.mark.parametrize("interleaved", [False, True], ids=["neox", "gptj"])
def test_elements_past_r_are_bit_copies(interleaved):
    d = 128
    x = _inputs(torch.bfloat16, (1, 2, 16, d), 3)
    for r in (16, 64, 96):
        cos, sin = rope_refs.rope_tables(32, r)
        y = rope_refs.rotate(x, cos[3:19][None, None], sin[3:19][None, None], interleaved)
        assert torch.equal(y[..., r:].view(torch.int16), x[..., r:].view(torch.int16))
        assert not torch.equal(y[..., :r].view(torch.int16), x[..., :r].view(torch.int16))


@pytest.mark.parametrize("sn", sorted(LENS))
def test_pos_is_the_appends_row(sn):
    """pos[b, t] is the row `expect_cache` (the append's rule) writes token t to."""
    lens = LENS[sn]
    pos, n = rope_refs.positions(lens, sn)
    assert n.tolist() == [sn] * 3
    cap = 256  # larger than every length: no row is dropped for the capacity
    cache = torch.full((3, 1, cap, 1), -1, dtype=torch.int32)
    src = torch.arange(sn, dtype=torch.int32).reshape(1, 1, sn, 1).expand(3, 1, sn, 1)
    out = rope_refs.expect_cache(cache, src, lens)[:, 0, :, 0]
    for b in range(3):
        for t in range(sn):
            r = int(pos[b, t])
            assert r == lens[b] - sn + t
            if r >= 0:
                assert int(out[b, r]) == t
        assert int((out[b] >= 0).sum()) == int((pos[b] >= 0).sum())
    # new_lens: clamped to [0, Sn]
    pos, n = rope_refs.positions((40, 66, 70), 16, (0, 20, -3))
    assert n.tolist() == [0, 16, 0] and pos[1].tolist() == list(range(50, 66))
    # rope_len: rows at or past it are dropped
    out = rope_refs.expect_cache(cache, src, lens, rope_len=100)[:, 0, :, 0]
    assert int((out[:, 100:] >= 0).sum()) == 0
