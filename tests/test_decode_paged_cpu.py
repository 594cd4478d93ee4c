"""CPU tests of the paged decode-attention entries (fa_decode_paged_f16 /
fa_decode_paged_bf16, fa_mi355x.flash_attention_decode_paged,
torch.ops.fa_mi355x.decode_paged): exports, the argument checks (all returned
before any launch, so fake pointers do), the Python wrapper's tensor checks,
the op's registration and the kernels' compile-time resource usage -- no
kernel is launched (no GPU here)."""
import os

import pytest
import torch

import capi_checks
from capi_checks import fa as _fa

SYMBOLS = ("fa_decode_paged_f16", "fa_decode_paged_bf16")


def test_library_exports_paged_symbols():
    capi_checks.assert_exported(SYMBOLS)


def test_argument_checks():
    fa = _fa()
    capi_checks.decode_paged_argument_checks(fa, fa.load_library())


def _t(shape, dtype=torch.float16, device="meta"):
    return torch.empty(shape, dtype=dtype, device=device)


def test_python_wrapper_rejects_bad_tensors():
    """Each rejection is raised by its own check: dtypes, ranks and shapes are
    checked before the device, so the message names the property that is wrong
    even though none of these tensors is on a GPU (device-side rejections:
    tests/test_decode_paged_gpu.py)."""
    fa = _fa()
    q, kp = (2, 8, 1, 128), (40, 2, 128, 128)
    i32 = torch.int32

    def tab(shape=(2, 4), dtype=i32):
        return _t(shape, dtype)

    bad = [
        ("q must be float16 or bfloat16",
         _t(q, torch.float32), _t(kp, torch.float32), _t(kp, torch.float32), tab(), None),
        ("q must be a device tensor", _t(q, device="cpu"), _t(kp, device="cpu"), _t(kp, device="cpu"),
         torch.zeros((2, 4), dtype=i32), None),
        ("q must be a device tensor", _t(q), _t(kp), _t(kp), tab(), None),
        ("k_pages and v_pages must have one shape", _t(q), _t(kp), _t((40, 2, 64, 128)), tab(), None),
        ("k_pages must be torch.float16", _t(q), _t(kp, torch.bfloat16), _t(kp), tab(), None),
        ("agree in head_dim", _t(q), _t((40, 2, 128, 64)), _t((40, 2, 128, 64)), tab(), None),
        ("q must be 4-D", _t((8, 1, 128)), _t(kp), _t(kp), tab(), None),
        ("k_pages must be 4-D", _t(q), _t((40, 2, 128 * 128)), _t(kp), tab(), None),
        ("v_pages must be contiguous", _t(q), _t(kp), _t((40, 2, 128, 128)).transpose(2, 3), tab(),
         None),
        ("the page pools hold no page", _t(q), _t((0, 2, 128, 128)), _t((0, 2, 128, 128)), tab(), None),
        ("page_size 96 is not a positive multiple of 64", _t(q), _t((40, 2, 96, 128)),
         _t((40, 2, 96, 128)), tab(), None),
        ("page_size 32 is not a positive multiple of 64", _t(q), _t((40, 2, 32, 128)),
         _t((40, 2, 32, 128)), tab(), None),
        ("page_size 0 is not a positive multiple of 64", _t(q), _t((40, 2, 0, 128)),
         _t((40, 2, 0, 128)), tab(), None),
        ("heads_q 7 is not a multiple of heads_kv 2", _t((2, 7, 1, 128)), _t(kp), _t(kp), tab(), None),
        ("block_table must be int32", _t(q), _t(kp), _t(kp), tab(dtype=torch.int64), None),
        ("block_table must be 2-D", _t(q), _t(kp), _t(kp), tab((8,)), None),
        ("block_table must be 2-D", _t(q), _t(kp), _t(kp), tab((2, 2, 2)), None),
        ("block_table has 3 rows, q a batch of 2", _t(q), _t(kp), _t(kp), tab((3, 4)), None),
        ("block_table must be contiguous", _t(q), _t(kp), _t(kp), tab((4, 2)).t(), None),
        ("kv_lens must be int32", _t(q), _t(kp), _t(kp), tab(), torch.zeros(2, dtype=torch.int64)),
        ("kv_lens must be a contiguous \\[B\\] tensor", _t(q), _t(kp), _t(kp), tab(),
         torch.zeros(3, dtype=i32)),
    ]
    for msg, tq, tk, tv, tt, lens in bad:
        with pytest.raises(fa.FlashAttentionError, match=msg):
            fa.flash_attention_decode_paged(tq, tk, tv, tt, lens, out=torch.empty_like(tq))


def test_decode_paged_op_registered_with_fake_impl():
    import fa_mi355x.torch_op as top

    assert top.DECODE_PAGED_OP_NAME == "fa_mi355x::decode_paged"
    schema = str(torch.ops.fa_mi355x.decode_paged.default._schema)
    assert schema == ("fa_mi355x::decode_paged(Tensor q, Tensor k_pages, Tensor v_pages, "
                      "Tensor block_table, Tensor? kv_lens=None, bool causal=True) -> Tensor"), schema
    for dtype in (torch.float16, torch.bfloat16):
        q = _t((2, 28, 3, 128), dtype)
        kp = _t((70, 4, 128, 128), dtype)
        table = _t((2, 32), torch.int32)
        lens = _t((2,), torch.int32)
        out = torch.ops.fa_mi355x.decode_paged(q, kp, kp, table, lens, True)
        assert out.shape == q.shape and out.dtype == dtype and out.device.type == "meta"
        assert torch.ops.fa_mi355x.decode_paged(q, kp, kp, table).shape == q.shape
    # no CPU path, forward only
    c = torch.zeros((1, 2, 1, 128), dtype=torch.float16)
    cp = torch.zeros((2, 2, 64, 128), dtype=torch.float16)
    with pytest.raises(ValueError):
        torch.ops.fa_mi355x.decode_paged(c, cp, cp, torch.zeros((1, 1), dtype=torch.int32))
    with pytest.raises(RuntimeError):
        torch.ops.fa_mi355x.decode_paged(_t((1, 2, 1, 128)).requires_grad_(), _t((2, 2, 64, 128)),
                                         _t((2, 2, 64, 128)), _t((1, 1), torch.int32))


@pytest.mark.skipif(not os.path.exists(capi_checks.HIPCC), reason="needs hipcc")
def test_no_paged_decode_kernel_uses_scratch():
    """Twin of test_decode_cpu.test_no_decode_kernel_uses_scratch for
    csrc/fa_decode_paged.hip: every paged decode kernel (2 dtypes x 2 head
    dims x 1 / 2 / 4 row blocks) keeps its state in registers."""
    (kernels,) = capi_checks.kernel_resource_usage(["fa_decode_paged.hip"])
    names = [n for n, _, _ in kernels]
    assert len(names) == 12, len(names)
    assert all("fa_decode_kernel" in n and "DecodePagedParams" in n for n in names), names
    spills = {n: s for n, s, _ in kernels if s}
    assert not spills, spills
