"""CPU tests of the paged decode-attention entries (fa_decode_paged_f16 /
fa_decode_paged_bf16, fa_mi355x.flash_attention_decode_paged,
torch.ops.fa_mi355x.decode_paged): exports, the argument checks (all returned
before any launch, so fake pointers do), the Python wrapper's tensor checks,
the op's registration and the kernels' compile-time resource usage -- no
kernel is launched (no GPU here)."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("fa_decode_paged_f16", "fa_decode_paged_bf16")
MAX_SPLITS = 64  # the plan's upper cap (csrc/fa_decode_host.hpp kDecodeMaxSplits)
INT_MAX = 2 ** 31 - 1


def _fa():
    import fa_mi355x

    return fa_mi355x


def test_library_exports_paged_symbols():
    fa = _fa()
    out = subprocess.run(["nm", "-D", "--defined-only", fa.library_path()], capture_output=True,
                         text=True, check=True).stdout
    syms = {line.split()[-1] for line in out.splitlines() if line.strip()}
    header = open(os.path.join(ROOT, "include", "fa_mi355x.h")).read()
    for s in SYMBOLS:
        assert s in syms, s
        assert s in fa.EXPORTED_SYMBOLS, s
        assert re.search(r"\b%s\s*\(" % s, header), s


def _call(fn, q, k, v, o, b, hq, hkv, sq, d, npages, psz, table, mpp, lens=None, causal=1, ns=0,
          ws=None, wsb=0):
    return fn(q, k, v, o, None, b, hq, hkv, sq, d, npages, psz, table, mpp, lens, causal, ns, ws, wsb,
              None)


def test_argument_checks():
    fa = _fa()
    lib = fa.load_library()
    p = ctypes.c_void_p(0x1000)
    for fn in (lib.fa_decode_paged_f16, lib.fa_decode_paged_bf16):
        # a good call's arguments: B=1 Hq=8 Hkv=2 Sq=1 D=128, 100 pages of 128 keys, 32 per sequence
        for bad in range(4):  # each of q, k_pages, v_pages, o NULL in turn
            ptrs = [None if i == bad else p for i in range(4)]
            assert _call(fn, *ptrs, 1, 8, 2, 1, 128, 100, 128, p, 32) == fa.FA_ERR_NULL_POINTER
        # a NULL table with a non-zero capacity
        assert _call(fn, p, p, p, p, 1, 8, 2, 1, 128, 100, 128, None, 32) == fa.FA_ERR_NULL_POINTER
        for psz in (0, 32, 96, -64, 1, 63, 65):
            assert _call(fn, p, p, p, p, 1, 8, 2, 1, 128, 100, psz, p, 32) == fa.FA_ERR_BAD_SHAPE, psz
        for npages in (0, -1):
            assert _call(fn, p, p, p, p, 1, 8, 2, 1, 128, npages, 128, p, 32) == fa.FA_ERR_BAD_SHAPE
        assert _call(fn, p, p, p, p, 1, 8, 2, 1, 128, 100, 128, p, -1) == fa.FA_ERR_BAD_SHAPE
        # logical capacity past INT_MAX - 64 (the last one at or below it is accepted as a shape:
        # it fails later, on the missing workspace of its split)
        assert (INT_MAX - 64) // 64 * 64 == 2147483520
        assert _call(fn, p, p, p, p, 1, 8, 2, 1, 128, 100, 64, p, 2147483520 // 64 + 1) == \
            fa.FA_ERR_BAD_SHAPE
        assert _call(fn, p, p, p, p, 1, 8, 2, 1, 128, 100, 64, p, 2147483520 // 64) == \
            fa.FA_ERR_WORKSPACE
        assert _call(fn, p, p, p, p, 1, 8, 2, 1, 128, 100, 1 << 20, p, 1 << 12) == fa.FA_ERR_BAD_SHAPE
        # one page's rows of a head past a 32-bit byte range
        assert _call(fn, p, p, p, p, 1, 8, 2, 1, 128, 1, 1 << 23, p, 1) == fa.FA_ERR_BAD_SHAPE
        # the contiguous entry's checks
        for d in (0, 32, 96, 256):
            assert _call(fn, p, p, p, p, 1, 8, 2, 1, d, 100, 128, p, 32) == \
                fa.FA_ERR_UNSUPPORTED_HEAD_DIM
        for hq, hkv in ((8, 3), (7, 2), (4, 8)):
            assert _call(fn, p, p, p, p, 1, hq, hkv, 1, 128, 100, 128, p, 32) == fa.FA_ERR_BAD_SHAPE
        for sq in (0, 17, -1):
            assert _call(fn, p, p, p, p, 1, 8, 2, sq, 128, 100, 128, p, 32) == fa.FA_ERR_BAD_SHAPE
        assert _call(fn, p, p, p, p, -1, 8, 2, 1, 128, 100, 128, p, 32) == fa.FA_ERR_BAD_SHAPE
        assert _call(fn, p, p, p, p, 1, -8, 2, 1, 128, 100, 128, p, 32) == fa.FA_ERR_BAD_SHAPE
        assert _call(fn, p, p, p, p, 1, 8, -2, 1, 128, 100, 128, p, 32) == fa.FA_ERR_BAD_SHAPE
        assert _call(fn, p, p, p, p, 1, 8, 2, 1, 128, 100, 128, p, 32, ns=-1) == fa.FA_ERR_BAD_SHAPE
        # splitting needs a workspace: present, long enough (fa_decode_ws_bytes with the
        # logical capacity 32 * 128), 16-byte aligned
        need = lib.fa_decode_ws_bytes(1, 8, 2, 1, 32 * 128, 128, 4)
        assert need > 65536
        assert _call(fn, p, p, p, p, 1, 8, 2, 1, 128, 100, 128, p, 32, ns=4) == fa.FA_ERR_WORKSPACE
        assert _call(fn, p, p, p, p, 1, 8, 2, 1, 128, 100, 128, p, 32, ns=4, ws=p, wsb=need - 1) == \
            fa.FA_ERR_WORKSPACE
        assert _call(fn, p, p, p, p, 1, 8, 2, 1, 128, 100, 128, p, 32, ns=4,
                     ws=ctypes.c_void_p(0x1008), wsb=need) == fa.FA_ERR_WORKSPACE
        # the plan's own split (num_splits = 0) of this shape needs one too
        assert lib.fa_decode_num_splits(1, 8, 2, 1, 32 * 128, 128) > 1
        assert _call(fn, p, p, p, p, 1, 8, 2, 1, 128, 100, 128, p, 32) == fa.FA_ERR_WORKSPACE
        # more pieces than the cap
        assert _call(fn, p, p, p, p, 1, 8, 2, 1, 128, 100, 128, p, 32, ns=MAX_SPLITS + 1, ws=p,
                     wsb=1 << 40) == fa.FA_ERR_BAD_CONFIG
        # empty problems: nothing to do, nothing launched, no pointer looked at
        assert _call(fn, None, None, None, None, 0, 8, 2, 1, 128, 100, 128, None, 32) == fa.FA_OK
        assert _call(fn, None, None, None, None, 1, 0, 0, 1, 128, 100, 128, None, 32) == fa.FA_OK
        # ... but the page geometry is still checked
        assert _call(fn, None, None, None, None, 0, 8, 2, 1, 128, 100, 96, None, 32) == \
            fa.FA_ERR_BAD_SHAPE


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


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_no_paged_decode_kernel_uses_scratch():
    """Twin of test_decode_cpu.test_no_decode_kernel_uses_scratch for
    csrc/fa_decode_paged.hip: every paged decode kernel (2 dtypes x 2 head
    dims x 1 / 2 / 4 row blocks) keeps its state in registers."""
    pkg = os.path.join(ROOT, "flash-attention-cuda_amd")
    cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fno-honor-nans",
           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(pkg, "csrc"), "-c",
           os.path.join(pkg, "csrc", "fa_decode_paged.hip"), "-o", os.devnull,
           "-Rpass-analysis=kernel-resource-usage"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", out.stderr)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", out.stderr)]
    assert len(names) == 12 and len(names) == len(scratch), (len(names), len(scratch))
    assert all("fa_decode_kernel" in n and "DecodePagedParams" in n for n in names), names
    spills = {n: s for n, s in zip(names, scratch) if s}
    assert not spills, spills
