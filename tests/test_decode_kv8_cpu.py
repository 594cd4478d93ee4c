"""CPU tests of the decode entries over an FP8 (E4M3) K/V cache
(fa_decode_kv8_f16 / _bf16, fa_decode_paged_kv8_f16 / _bf16, the k_scale /
v_scale arguments of fa_mi355x.flash_attention_decode[_paged] and of the torch
ops): exports, the 16-bit entries' argument-check tables run against the new
entries, the wrapper's rejections, the ops' schemas and fake implementations,
the exactness of E4M3 -> fp16 / bf16, and the kernels' compile-time resource
usage -- no kernel is launched (no GPU here)."""
import ctypes
import os

import pytest
import torch

import capi_checks
from capi_checks import fa as _fa

SYMBOLS = ("fa_decode_kv8_f16", "fa_decode_kv8_bf16", "fa_decode_paged_kv8_f16",
           "fa_decode_paged_kv8_bf16")
FP8 = torch.float8_e4m3fn


def test_library_exports_kv8_symbols():
    capi_checks.assert_exported(SYMBOLS)


class _Kv8Lib:
    """The loaded library with the 16-bit decode entries' names bound to the
    kv8 entries (the two scale pointers appended), everything else as it is:
    the 16-bit entries' argument tables then run against the new entries."""

    def __init__(self, lib, scales):
        self._lib = lib
        for old, new in (("fa_decode_f16", "fa_decode_kv8_f16"),
                         ("fa_decode_bf16", "fa_decode_kv8_bf16"),
                         ("fa_decode_paged_f16", "fa_decode_paged_kv8_f16"),
                         ("fa_decode_paged_bf16", "fa_decode_paged_kv8_bf16")):
            fn = getattr(lib, new)
            setattr(self, old, lambda *a, _fn=fn: _fn(*a, *scales))

    def __getattr__(self, name):
        return getattr(self._lib, name)


ARGUMENT_TABLES = {"test_decode_cpu.py": capi_checks.decode_argument_checks,
                   "test_decode_paged_cpu.py": capi_checks.decode_paged_argument_checks}


@pytest.mark.parametrize("scales", [(None, None), (ctypes.c_void_p(0x2000), ctypes.c_void_p(0x3000)),
                                    (None, ctypes.c_void_p(0x3000))],
                         ids=["null-scales", "scales", "v-scale-only"])
@pytest.mark.parametrize("fname", list(ARGUMENT_TABLES))
def test_argument_checks(fname, scales):
    """The same status codes in the same order as the 16-bit twins (fname: the
    file whose test_argument_checks runs the same table against the 16-bit
    entries), all before any launch (fake pointers), whatever the scale
    pointers are."""
    fa = _fa()
    ARGUMENT_TABLES[fname](fa, _Kv8Lib(fa.load_library(), scales))


def _t(shape, dtype=torch.float16, device="meta"):
    return torch.empty(shape, dtype=dtype, device=device)


def test_python_wrapper_rejections():
    """One rejection per cause, each raised before the device is looked at
    (meta tensors); an accepted FP8 call gets as far as the device check."""
    fa = _fa()
    q, k, kp = (2, 8, 1, 128), (2, 2, 512, 128), (40, 2, 128, 128)
    f32 = torch.float32
    ok_s = _t((2,), f32)
    bad = [
        # (message, k dtype, v dtype, k_scale, v_scale)
        ("must have one dtype, got torch.float8_e4m3fn and torch.float16", FP8, torch.float16, None, None),
        ("must have one dtype, got torch.float16 and torch.float8_e4m3fn", torch.float16, FP8, ok_s, None),
        ("torch.float8_e4m3fnuz is not supported", torch.float8_e4m3fnuz, torch.float8_e4m3fnuz, None, None),
        ("torch.float8_e5m2 is not supported", torch.float8_e5m2, torch.float8_e5m2, ok_s, ok_s),
        ("must have one dtype, got torch.float8_e4m3fn and torch.float8_e5m2", FP8, torch.float8_e5m2,
         None, None),
        ("(v_cache|v_pages): torch.float8_e5m2 is not supported", torch.float16, torch.float8_e5m2, None, None),
        ("must be torch.float16, got torch.int8", torch.int8, torch.int8, None, None),
        ("must be torch.float16, got torch.uint8", torch.uint8, torch.uint8, ok_s, ok_s),
        ("must be torch.float16, got torch.bfloat16", torch.bfloat16, torch.float16, None, None),
        ("go with a torch.float8_e4m3fn cache only", torch.float16, torch.float16, ok_s, None),
        ("go with a torch.float8_e4m3fn cache only", torch.float16, torch.float16, None, ok_s),
        ("k_scale must be a contiguous float32 \\[Hkv = 2\\] tensor", FP8, FP8, _t((3,), f32), None),
        ("v_scale must be a contiguous float32 \\[Hkv = 2\\] tensor", FP8, FP8, ok_s, _t((2,), torch.float16)),
        ("k_scale must be a contiguous float32 \\[Hkv = 2\\] tensor", FP8, FP8, _t((2, 1), f32), None),
        ("v_scale must be a contiguous float32 \\[Hkv = 2\\] tensor", FP8, FP8, None, _t((4,), f32)[::2]),
        ("k_scale must be a contiguous float32 \\[Hkv = 2\\] tensor", FP8, FP8, 0.5, None),
        # nothing wrong but the device: the FP8 cache and its scales were accepted
        ("q must be a device tensor", FP8, FP8, ok_s, ok_s),
        ("q must be a device tensor", FP8, FP8, None, None),
    ]
    tab = _t((2, 4), torch.int32)
    for msg, kd, vd, ks, vs in bad:
        for name in ("k_cache", "k_pages"):
            full = msg if not msg.startswith("must ") or "one dtype" in msg else name + " " + msg
            with pytest.raises(fa.FlashAttentionError, match=full):
                if name == "k_cache":
                    fa.flash_attention_decode(_t(q), _t(k, kd), _t(k, vd), None, out=_t(q),
                                              k_scale=ks, v_scale=vs)
                else:
                    fa.flash_attention_decode_paged(_t(q), _t(kp, kd), _t(kp, vd), tab, None, out=_t(q),
                                                    k_scale=ks, v_scale=vs)
    # bf16 q: the 16-bit message names q's dtype; out stays q's dtype beside an FP8 cache
    with pytest.raises(fa.FlashAttentionError, match="k_cache must be torch.bfloat16, got torch.float16"):
        fa.flash_attention_decode(_t(q, torch.bfloat16), _t(k), _t(k), None, out=_t(q, torch.bfloat16))
    with pytest.raises(fa.FlashAttentionError, match="out must be torch.float16"):
        fa.flash_attention_decode(_t(q), _t(k, FP8), _t(k, FP8), None, out=_t(q, FP8))


def test_scales_on_another_device_are_rejected():
    """The scales' own device check (the wrappers run it last, after q's, the
    caches' and out's: tests/test_decode_kv8_gpu.py has a host scale beside
    device tensors)."""
    fa = _fa()
    q = _t((2, 8, 1, 128))
    with pytest.raises(fa.FlashAttentionError, match="k_scale must be a tensor on"):
        fa._check_scales_device(q, torch.ones(2), None)
    with pytest.raises(fa.FlashAttentionError, match="v_scale must be a tensor on"):
        fa._check_scales_device(q, None, torch.ones(2))


def test_ops_take_fp8_caches_and_scales():
    import fa_mi355x.torch_op as top  # noqa: F401

    schema = str(torch.ops.fa_mi355x.decode.default._schema)
    assert "Tensor? kv_lens=None" in schema and "bool causal=True" in schema, schema
    assert schema.endswith("Tensor? k_scale=None, Tensor? v_scale=None) -> Tensor"), schema
    # the paged op: the default overload as it was, the scales in the kv8 overload
    assert str(torch.ops.fa_mi355x.decode_paged.default._schema) == (
        "fa_mi355x::decode_paged(Tensor q, Tensor k_pages, Tensor v_pages, "
        "Tensor block_table, Tensor? kv_lens=None, bool causal=True) -> Tensor")
    assert str(torch.ops.fa_mi355x.decode_paged.kv8._schema) == (
        "fa_mi355x::decode_paged.kv8(Tensor q, Tensor k_pages, Tensor v_pages, "
        "Tensor block_table, Tensor? kv_lens=None, bool causal=True, Tensor? k_scale=None, "
        "Tensor? v_scale=None) -> Tensor")
    lens = _t((2,), torch.int32)
    tab = _t((2, 32), torch.int32)
    ks = _t((4,), torch.float32)
    for dtype in (torch.float16, torch.bfloat16):
        q = _t((2, 28, 3, 128), dtype)
        k = _t((2, 4, 4096, 128), FP8)
        kp = _t((80, 4, 128, 128), FP8)
        outs = [
            torch.ops.fa_mi355x.decode(q, k, k),
            torch.ops.fa_mi355x.decode(q, k, k, lens, True),           # the positional call of before
            torch.ops.fa_mi355x.decode(q, k, k, lens, True, ks, ks),
            torch.ops.fa_mi355x.decode(q, k, k, k_scale=ks),
            torch.ops.fa_mi355x.decode_paged(q, kp, kp, tab),
            torch.ops.fa_mi355x.decode_paged(q, kp, kp, tab, lens, True),
            torch.ops.fa_mi355x.decode_paged(q, kp, kp, tab, lens, True, ks, ks),
            torch.ops.fa_mi355x.decode_paged(q, kp, kp, tab, v_scale=ks),
            torch.ops.fa_mi355x.decode_paged.kv8(q, kp, kp, tab, lens, True, ks, None),
        ]
        for out in outs:
            assert out.shape == q.shape and out.dtype == dtype and out.device.type == "meta"
    c = torch.zeros((1, 2, 1, 128), dtype=torch.float16)
    c8 = torch.zeros((1, 2, 8, 128), dtype=torch.float16).to(FP8)
    with pytest.raises(ValueError):  # no CPU path
        torch.ops.fa_mi355x.decode(c, c8, c8, None, True, torch.ones(2), None)
    with pytest.raises(ValueError):
        torch.ops.fa_mi355x.decode_paged(c, c8, c8, torch.zeros((1, 1), dtype=torch.int32), None, True,
                                         torch.ones(2), None)


def test_e4m3_is_exact_in_fp16_and_bf16():
    """All 254 finite E4M3 codes (0x7f and 0xff are NaN, there is no infinity)
    convert to fp16 and to bf16 and back without change: the kernel's
    conversion of the cache loses nothing."""
    codes = torch.arange(256, dtype=torch.int16).to(torch.uint8)
    f8 = codes.view(FP8)
    val = f8.float()
    finite = torch.isfinite(val)
    assert int(finite.sum()) == 254 and not bool(finite[0x7f]) and not bool(finite[0xff])
    assert float(val[finite].abs().max()) == 448.0
    assert float(val[finite][val[finite] != 0].abs().min()) == 2.0 ** -9
    for dt in (torch.float16, torch.bfloat16):
        mid = f8.to(dt)
        assert torch.equal(mid.float()[finite], val[finite]), dt
        back = mid.to(FP8).view(torch.uint8)
        assert torch.equal(back[finite], codes[finite]), dt  # -0.0 (0x80) keeps its sign
        assert bool(torch.isnan(mid[~finite].float()).all()), dt


@pytest.mark.skipif(not os.path.exists(capi_checks.HIPCC), reason="needs hipcc")
def test_no_kv8_kernel_uses_scratch():
    """2 dtypes x 2 head dims x 1 / 2 / 4 row blocks x contiguous / paged = 24
    kv8 kernels, every one with its state in registers."""
    units = ("fa_decode_kv8.hip", "fa_decode_paged_kv8.hip")
    total = 0
    for unit, kernels in zip(units, capi_checks.kernel_resource_usage(units, timeout=900)):
        names = [n for n, _, _ in kernels]
        assert len(names) == 12, (unit, len(names))
        paged = "paged" in unit
        want = "DecodePagedKv8Params" if paged else "DecodeKv8Params"
        assert all("fa_decode_kernel" in n and want in n for n in names), names
        spills = {n: s for n, s, _ in kernels if s}
        assert not spills, spills
        total += len(names)
    assert total == 24
