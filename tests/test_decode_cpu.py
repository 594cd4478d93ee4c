"""CPU tests of the decode-attention entries (fa_decode_f16 / fa_decode_bf16,
fa_decode_num_splits, fa_decode_ws_bytes, fa_mi355x.flash_attention_decode,
torch.ops.fa_mi355x.decode): exports, the argument checks (all returned before
any launch, so fake pointers do), the split plan, the workspace size, the
Python wrapper's tensor checks, the op's registration and the kernels'
compile-time resource usage -- no kernel is launched (no GPU here)."""
import os

import pytest
import torch

import capi_checks
from capi_checks import MAX_SPLITS, fa as _fa

SYMBOLS = ("fa_decode_f16", "fa_decode_bf16", "fa_decode_num_splits", "fa_decode_ws_bytes")


def test_library_exports_decode_symbols():
    capi_checks.assert_exported(SYMBOLS)


def test_argument_checks():
    fa = _fa()
    capi_checks.decode_argument_checks(fa, fa.load_library())


def test_eight_entries_answer_shared_arguments_alike():
    """The contiguous, paged, FP8 and paged FP8 entries (f16 and bf16 each) run
    one host body (csrc/fa_decode_host.hpp): a violation of an argument they
    share gets the same status from all eight, in the same precedence.  Every
    pointer is NULL, so nothing can launch; the family's own arguments are valid
    (kv_capacity 256, or 4 pages of 64 keys with 4 table entries per row)."""
    fa = _fa()
    lib = fa.load_library()
    base = dict(batch=2, heads_q=8, heads_kv=2, seqlen_q=1, head_dim=128, num_splits=0)
    shape, dim, ok, null = (fa.FA_ERR_BAD_SHAPE, fa.FA_ERR_UNSUPPORTED_HEAD_DIM, fa.FA_OK,
                            fa.FA_ERR_NULL_POINTER)
    rows = [({name: -1}, shape) for name in ("batch", "heads_q", "heads_kv", "head_dim", "num_splits")]
    rows += [
        (dict(head_dim=96), dim), (dict(head_dim=0), dim),
        (dict(seqlen_q=0), shape), (dict(seqlen_q=17), shape),
        (dict(batch=0), ok), (dict(heads_q=0), ok),
        (dict(heads_kv=0), shape), (dict(heads_kv=3), shape),
        (dict(batch=1 << 20, heads_q=1 << 12, heads_kv=1), shape),  # rows past INT_MAX
        ({}, null),
        # precedence
        (dict(head_dim=96, seqlen_q=0), dim),
        (dict(batch=0, seqlen_q=17), shape),
        (dict(batch=0, heads_kv=0), ok),
    ]

    def statuses(batch, heads_q, heads_kv, seqlen_q, head_dim, num_splits):
        n5, bhhs = (None,) * 5, (batch, heads_q, heads_kv, seqlen_q)
        end = (None, 1, num_splits, None, 0, None)  # kv_lens, causal, num_splits, ws, ws_bytes, stream
        contig = n5 + bhhs + (256, head_dim) + end
        # head_dim, num_pages, page_size, block_table, max_pages_per_seq
        paged = n5 + bhhs + (head_dim, 4, 64, None, 4) + end
        return [getattr(lib, "fa_decode" + fam + dt)(*args)
                for fam, args in (("", contig), ("_paged", paged), ("_kv8", contig + (None, None)),
                                  ("_paged_kv8", paged + (None, None)))
                for dt in ("_f16", "_bf16")]

    for change, want in rows:
        got = statuses(**dict(base, **change))
        assert len(got) == 8 and got == [want] * 8, (change, want, got)


def test_split_plan():
    """fa_decode_num_splits without a device: the default 256 CUs."""
    lib = _fa().load_library()
    ns = lib.fa_decode_num_splits
    # units already fill (twice) the CUs: one piece
    for b, hkv in ((64, 8), (512, 1), (16, 32)):
        assert b * hkv >= 2 * 256
        assert ns(b, 4 * hkv, hkv, 1, 32768, 128) == 1, (b, hkv)
    assert ns(1, 32, 8, 1, 32768, 128) > 1
    for cap in (1, 100, 255, 256, 257, 1000, 4096, 32768, 1 << 20):
        for b, hq, hkv, sq in ((1, 32, 8, 1), (1, 8, 1, 1), (8, 32, 8, 4), (1, 28, 4, 16), (3, 7, 7, 2)):
            for d in (64, 128):
                n = ns(b, hq, hkv, sq, cap, d)
                assert 1 <= n <= MAX_SPLITS, (b, hq, hkv, sq, cap, d, n)
                assert n <= -(-cap // 256), (b, hq, hkv, sq, cap, d, n)
    # the longest cache of the fewest units still stays under the cap
    assert ns(1, 1, 1, 1, 8388607, 128) == MAX_SPLITS


def test_workspace_bytes():
    lib = _fa().load_library()
    wsb = lib.fa_decode_ws_bytes
    # the plan does not split: no workspace
    assert lib.fa_decode_num_splits(64, 32, 8, 1, 32768, 128) == 1
    assert wsb(64, 32, 8, 1, 32768, 128, 0) == 0
    assert wsb(1, 32, 8, 1, 100, 128, 0) == 0      # too short to split
    assert wsb(1, 32, 8, 1, 32768, 128, 1) == 0    # one forced piece
    for shape in ((1, 32, 8, 1, 32768, 128), (8, 32, 8, 4, 8192, 128), (1, 28, 4, 3, 4096, 64),
                  (2, 16, 1, 16, 2048, 128)):
        assert lib.fa_decode_num_splits(*shape) > 1, shape
        need = wsb(*shape, 0)
        assert need >= 65536 and need % 256 == 0, shape
        assert need == wsb(*shape, lib.fa_decode_num_splits(*shape))
        prev = 0
        for forced in range(2, MAX_SPLITS + 1):
            n = wsb(*shape, forced)
            assert n >= 65536 and n % 256 == 0 and n > prev, (shape, forced)
            prev = n


def _t(shape, dtype=torch.float16, device="meta"):
    return torch.empty(shape, dtype=dtype, device=device)


def test_python_wrapper_rejects_bad_tensors():
    """Each rejection is raised by its own check: dtypes, ranks and shapes are
    checked before the device, so the message names the property that is wrong
    even though none of these tensors is on a GPU (a host kv_lens beside
    device tensors: tests/test_decode_gpu.py)."""
    fa = _fa()
    q, k = (2, 8, 1, 128), (2, 2, 512, 128)
    bad = [
        ("q must be float16 or bfloat16",
         _t(q, torch.float32), _t(k, torch.float32), _t(k, torch.float32), None),
        ("q must be a device tensor", _t(q, device="cpu"), _t(k, device="cpu"), _t(k, device="cpu"), None),
        ("q must be a device tensor", _t(q), _t(k), _t(k), None),
        ("k_cache and v_cache must have one shape", _t(q), _t(k), _t((2, 2, 256, 128)), None),
        ("kv_lens must be int32", _t(q), _t(k), _t(k), torch.zeros(2, dtype=torch.int64)),
        ("kv_lens must be a contiguous \\[B\\] tensor", _t(q), _t(k), _t(k),
         torch.zeros(3, dtype=torch.int32)),
        ("heads_q 7 is not a multiple of heads_kv 2", _t((2, 7, 1, 128)), _t(k), _t(k), None),
        ("k_cache must be torch.float16", _t(q), _t(k, torch.bfloat16), _t(k), None),
        ("agree in batch and head_dim", _t(q), _t((3, 2, 512, 128)), _t((3, 2, 512, 128)), None),
        ("agree in batch and head_dim", _t(q), _t((2, 2, 512, 64)), _t((2, 2, 512, 64)), None),
        ("q must be 4-D", _t((8, 1, 128)), _t(k), _t(k), None),
        ("v_cache must be contiguous", _t(q), _t(k), _t((2, 2, 128, 512)).transpose(2, 3), None),
    ]
    for msg, tq, tk, tv, lens in bad:
        with pytest.raises(fa.FlashAttentionError, match=msg):
            fa.flash_attention_decode(tq, tk, tv, lens, out=torch.empty_like(tq))


def test_decode_op_registered_with_fake_impl():
    import fa_mi355x.torch_op as top

    assert top.DECODE_OP_NAME == "fa_mi355x::decode"
    schema = str(torch.ops.fa_mi355x.decode.default._schema)
    assert "Tensor? kv_lens=None" in schema and "bool causal=True" in schema, schema
    for dtype in (torch.float16, torch.bfloat16):
        q = _t((2, 28, 3, 128), dtype)
        k = _t((2, 4, 4096, 128), dtype)
        lens = torch.empty(2, dtype=torch.int32, device="meta")
        out = torch.ops.fa_mi355x.decode(q, k, k, lens, True)
        assert out.shape == q.shape and out.dtype == dtype and out.device.type == "meta"
        assert torch.ops.fa_mi355x.decode(q, k, k).shape == q.shape
    # no CPU path, forward only
    c = torch.zeros((1, 2, 1, 128), dtype=torch.float16)
    with pytest.raises(ValueError):
        torch.ops.fa_mi355x.decode(c, c, c)
    with pytest.raises(RuntimeError):
        torch.ops.fa_mi355x.decode(_t((1, 2, 1, 128)).requires_grad_(), _t((1, 2, 8, 128)),
                                   _t((1, 2, 8, 128)))


@pytest.mark.skipif(not os.path.exists(capi_checks.HIPCC), reason="needs hipcc")
def test_no_decode_kernel_uses_scratch():
    """Twin of test_capi.test_no_kernel_uses_scratch for csrc/fa_decode.hip:
    every decode kernel (2 dtypes x 2 head dims x 1 / 2 / 4 row blocks) keeps
    its state in registers."""
    (kernels,) = capi_checks.kernel_resource_usage(["fa_decode.hip"])
    names = [n for n, _, _ in kernels]
    assert len(names) == 12, len(names)
    assert all("fa_decode_kernel" in n for n in names), names
    spills = {n: s for n, s, _ in kernels if s}
    assert not spills, spills
