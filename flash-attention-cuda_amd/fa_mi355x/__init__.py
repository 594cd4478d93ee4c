"""fa_mi355x -- Python host side of the MI355X flash-attention forward path.

A thin ctypes binding over the C ABI in ``include/fa_mi355x.h`` (the drop-in
for the reference's ``flash_attention_v9_dispatch``,
/root/reference/flash_attention.cu:606-663).  PyTorch supplies device memory
and the current HIP stream; all arithmetic runs in the hand-written gfx950
kernels of ``libfa_mi355x.so``.  There is no fallback: if the library is
missing, every entry point raises :class:`FlashAttentionError`.
"""
from __future__ import annotations

import ctypes
import os
from dataclasses import dataclass
from typing import List, Optional

_HERE = os.path.dirname(os.path.abspath(__file__))
PKG_ROOT = os.path.dirname(_HERE)
# FA_MI355X_LIB: another in-tree build of the library (experiment variants,
# tools/w4_variant.sh) for a test or tool run; default the product library
LIB_PATH = os.environ.get("FA_MI355X_LIB") or os.path.join(PKG_ROOT, "lib", "libfa_mi355x.so")

HEAD_DIM = 128

FA_OK = 0
FA_ERR_NULL_POINTER = 1
FA_ERR_UNSUPPORTED_HEAD_DIM = 2
FA_ERR_BAD_SHAPE = 3
FA_ERR_LAUNCH = 4
FA_ERR_BAD_CONFIG = 5
FA_ERR_HIP = 6
FA_ERR_WORKSPACE = 7

FA_DTYPE_F16 = 0
FA_DTYPE_BF16 = 1


class FlashAttentionError(RuntimeError):
    """Raised for a nonzero fa_status_t (the reference exit()s instead)."""

    def __init__(self, status: int, msg: str):
        super().__init__(f"fa_mi355x error {status}: {msg}")
        self.status = status


class _ConfigInfo(ctypes.Structure):
    _fields_ = [
        ("id", ctypes.c_int),
        ("block_m", ctypes.c_int),
        ("block_n", ctypes.c_int),
        ("waves", ctypes.c_int),
        ("causal", ctypes.c_int),
        ("split_kv", ctypes.c_int),
        ("lds_bytes", ctypes.c_int),
        ("name", ctypes.c_char_p),
        ("dtype", ctypes.c_int),
        ("head_dim", ctypes.c_int),
    ]


class _KernelAttrs(ctypes.Structure):
    _fields_ = [
        ("num_regs", ctypes.c_int),
        ("local_size_bytes", ctypes.c_int),
        ("shared_size_bytes", ctypes.c_int),
        ("max_threads_per_block", ctypes.c_int),
        ("blocks_per_cu", ctypes.c_int),
    ]


_I, _P, _LL, _ULL = ctypes.c_int, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_ulonglong

# The launch entries' argument groups, as the macros that stamp the entries on
# the C side name them (csrc/fa_decode_host.hpp): a family below is one line of
# groups in C order, and no list is made from another entry's list.
_QKVO_LSE = [_P] * 5               # q, k, v, o, lse
_CACHE = {"": [_I, _I],            # CONTIG: kv_capacity, head_dim
          "_paged": [_I, _I, _I, _P, _I]}  # PAGED: head_dim, num_pages, page_size, block_table, max_pages_per_seq
_WINDOW = {"": [], "_win": [_I], "_sink": [_I]}       # PLAIN | WIN | SINK: window
_SINKS = {"": [], "_win": [], "_sink": [_P]}          # ... sinks
_BWD_SINKS = {"": [], "_win": [], "_sink": [_P, _P]}  # ... sinks, dsinks (the backward)
_SCALES = {"": [], "_kv8": [_P, _P]}                  # KV16 | KV8: k_scale, v_scale
_TREE_MASK = [_P]                                     # TREE: tree_mask, after sinks
_APPEND_HEAD = [_P] * 4 + [_I] * 3  # k_new, v_new, k_cache, v_cache, batch, heads_kv, seqlen_new / total_new
_ROPE_TAIL = [_P, _P, _I, _P, _P, _I, _I, _I]  # q, q_out, heads_q, cos, sin, rope_len, rotary_dim, interleaved
_STRIDES = [_LL] * 3               # the token strides of q, k, v
_BWD_PTRS = [_P] * 10              # dout, q, k, v, out, lse, dq, dk, dv, delta
_ATTN_DIMS = [_I] * 6              # batch, heads_q, heads_kv, total_q, total_k, head_dim
_ATTN_SEQS = [_P, _P, _I, _I, _I]  # cu_seqlens_q, cu_seqlens_k, seqlen_q, seqlen_k, causal
_STREAM = [_P]
# the families whose two 16-bit cache forms have one entry for both element types, `_16`
_ONE_16 = ("fa_cache_append", "fa_cache_append_varlen")


def _c_entries():
    """name -> (restype, argtypes) of every function include/fa_mi355x.h declares."""
    fwd = [_P] * 4 + [_I] * 5  # q, k, v, o, batch, heads, seq_len, head_dim, causal
    table = {
        "fa_fwd_f16": (_I, fwd + _STREAM),
        "fa_fwd_bf16": (_I, fwd + _STREAM),
        "fa_fwd_f16_config": (_I, fwd + [_I] + _STREAM),
        "fa_fwd_bf16_config": (_I, fwd + [_I] + _STREAM),
        "fa_fwd_f16_splitkv": (_I, fwd + [_I, _P, _P] + _STREAM),
        "fa_splitkv_num_splits": (_I, [_I] * 4),
        "fa_splitkv_o_bytes": (_ULL, [_I] * 5),
        "fa_splitkv_ml_bytes": (_ULL, [_I] * 5),
        "fa_fwd_f16_ws": (_I, fwd + [_I, _P, _ULL] + _STREAM),
        "fa_fwd_bf16_ws": (_I, fwd + [_I, _P, _ULL] + _STREAM),
        "fa_fwd_ws_bytes": (_ULL, [_I] * 6),
        "fa_fwd_split_pieces": (_I, [_I] * 5),
        "fa_decode_num_splits": (_I, [_I] * 6),
        "fa_decode_ws_bytes": (_ULL, [_I] * 7),
        "fa_select_config": (_I, [_I] * 4),
        "fa_num_configs": (_I, []),
        "fa_config_info": (_I, [_I, ctypes.POINTER(_ConfigInfo)]),
        "fa_kernel_attrs": (_I, [_I, ctypes.POINTER(_KernelAttrs)]),
        "fa_status_string": (ctypes.c_char_p, [_I]),
        "fa_version": (ctypes.c_char_p, []),
    }
    plain, variants = ("",), ("", "_win", "_sink")
    no_cache = (("", ""),)
    caches = tuple((c, s) for c in ("", "_paged") for s in ("", "_kv8"))

    def bwd(v, c, s):  # (dout's stride before the three)
        return _BWD_PTRS + _ATTN_DIMS + [_LL] + _STRIDES + _ATTN_SEQS + _WINDOW[v] + _STREAM + _BWD_SINKS[v]

    # families, variants, cache forms, and the arguments of variant v over cache form c with scales s
    for families, vs, forms, args in (
        (("fa_decode",), variants, caches, lambda v, c, s: (
            _QKVO_LSE + [_I] * 4 + _CACHE[c] + [_P, _I] + _WINDOW[v] + _SINKS[v] + [_I, _P, _ULL] + _STREAM
            + _SCALES[s])),  # (batch, heads_q, heads_kv, seqlen_q; kv_lens, causal; num_splits, ws, ws_bytes)
        (("fa_prefill", "fa_prefill_varlen"), variants, caches, lambda v, c, s: (
            _QKVO_LSE + [_I] * 4 + _CACHE[c] + [_P, _P, _I] + _WINDOW[v] + _SINKS[v] + _STREAM
            + _SCALES[s])),  # (...; kv_lens, q_lens / cu_seqlens_q, causal)
        (_ONE_16, plain, caches, lambda v, c, s: (
            _APPEND_HEAD + _CACHE[c] + [_P, _P] + _STREAM + _SCALES[s])),  # (kv_lens, new_lens / cu_seqlens)
        (("fa_rope_append", "fa_rope_append_varlen"), plain, caches, lambda v, c, s: (
            _APPEND_HEAD + _CACHE[c] + [_P, _P] + _STREAM + _SCALES[s] + _ROPE_TAIL)),
        (("fa_attn_varlen",), variants, no_cache, lambda v, c, s: (
            _QKVO_LSE + _ATTN_DIMS + _STRIDES + _ATTN_SEQS + _WINDOW[v] + _STREAM + _SINKS[v])),
        (("fa_attn_varlen_bwd",), plain, no_cache, bwd),
        (("fa_attn_bwd",), ("_win", "_sink"), no_cache, bwd),
    ):
        for family in families:
            for v in vs:
                for c, s in forms:
                    for ty in ("_16",) if family in _ONE_16 and not s else ("_f16", "_bf16"):
                        table[family + v + c + s + ty] = (_I, args(v, c, s))  # as _entry_name composes it
    return table


# every function include/fa_mi355x.h declares: name -> (restype, argtypes); the
# tests check it against the header and that the .so exports every name
C_ENTRIES = _c_entries()
EXPORTED_SYMBOLS = tuple(C_ENTRIES)


def _tree_entries():
    """name -> (restype, argtypes) of every function include/fa_mi355x_tree.h
    declares: the `_sink` decode lists with `tree_mask` directly after `sinks`."""
    return {"fa_decode_tree" + c + s + ty: (_I, (
                _QKVO_LSE + [_I] * 4 + _CACHE[c] + [_P, _I] + _WINDOW["_sink"] + _SINKS["_sink"] + _TREE_MASK
                + [_I, _P, _ULL] + _STREAM + _SCALES[s]))
            for c in ("", "_paged") for s in ("", "_kv8") for ty in ("_f16", "_bf16")}


# the tree-masked decode entries (speculative-decoding verification), a table
# of their own beside a header of their own: C_ENTRIES stays fa_mi355x.h's
TREE_ENTRIES = _tree_entries()


@dataclass(frozen=True)
class TileConfig:
    id: int
    block_m: int
    block_n: int
    waves: int
    causal: bool
    split_kv: bool
    lds_bytes: int
    name: str
    dtype: str = "float16"  # element type of Q/K/V/O: "float16" or "bfloat16"
    head_dim: int = 128


_lib = None


def library_path() -> str:
    return LIB_PATH


def load_library() -> ctypes.CDLL:
    """Load libfa_mi355x.so (in-tree build). Raises loudly when absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise FlashAttentionError(
            FA_ERR_HIP,
            f"{LIB_PATH} not built (run `make -C {PKG_ROOT}` or __graft_entry__.build())",
        )
    lib = ctypes.CDLL(LIB_PATH)
    for table in (C_ENTRIES, TREE_ENTRIES):
        for name, (restype, argtypes) in table.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = restype, argtypes
    _lib = lib
    return lib


def _check(status: int) -> None:
    if status != FA_OK:
        msg = load_library().fa_status_string(status).decode()
        raise FlashAttentionError(status, msg)


def version() -> str:
    return load_library().fa_version().decode()


def configs() -> List[TileConfig]:
    lib = load_library()
    out = []
    for cid in range(lib.fa_num_configs()):
        ci = _ConfigInfo()
        _check(lib.fa_config_info(cid, ctypes.byref(ci)))
        out.append(
            TileConfig(ci.id, ci.block_m, ci.block_n, ci.waves, bool(ci.causal),
                       bool(ci.split_kv), ci.lds_bytes, ci.name.decode(),
                       "bfloat16" if ci.dtype == FA_DTYPE_BF16 else "float16", ci.head_dim)
        )
    return out


def select_config(batch: int, heads: int, seq_len: int, causal: bool) -> int:
    return load_library().fa_select_config(batch, heads, seq_len, int(bool(causal)))


def kernel_attrs(config_id: int) -> dict:
    ka = _KernelAttrs()
    _check(load_library().fa_kernel_attrs(config_id, ctypes.byref(ka)))
    return {f: getattr(ka, f) for f, _ in _KernelAttrs._fields_}


_DTYPES_16 = ()  # (torch.float16, torch.bfloat16) once torch is imported (lazily)


def _raw_stream(stream, dev: int) -> int:
    """Raw hipStream_t of `stream` (None: torch's current stream on device `dev`)."""
    if stream is None:
        import torch

        return torch._C._cuda_getCurrentRawStream(dev)
    return stream if isinstance(stream, int) else stream.cuda_stream


def _entry(name: str):
    """The C function `name` of the CURRENT library: looked up on the library
    object at every call (its own attribute cache dies with it), so a tool that
    swaps `_lib` is followed by every function here."""
    return getattr(_lib or load_library(), name)


def _entry_name(family: str, variant: str, paged, kv8, bf16) -> str:
    """The launch entry of a family ("fa_decode"), a variant ("", "_win",
    "_sink": :func:`_entry_variant`), a cache form and q's element type."""
    return (family + variant + ("_paged" if paged else "") + ("_kv8" if kv8 else "")
            + ("_16" if family in _ONE_16 and not kv8 else "_bf16" if bf16 else "_f16"))


def _cache_args(k, head_dim: int, block_table) -> tuple:
    """The entries' cache group: k a contiguous [B,Hkv,cap,D] cache (no block
    table) or a [num_pages,Hkv,page_size,D] pool."""
    if block_table is None:
        return (k.shape[2], head_dim)
    return (head_dim, k.shape[0], k.shape[2], block_table.data_ptr(), block_table.shape[1])


def _scale_args(kv8, k_scale, v_scale) -> tuple:
    """The kv8 entries' scales group, after the stream (None: 1.0)."""
    if not kv8:
        return ()
    return (k_scale.data_ptr() if k_scale is not None else None,
            v_scale.data_ptr() if v_scale is not None else None)


def _launch(name: str, dev: int, stream, before: tuple, after: tuple = ()) -> None:
    """Every launch but flash_attention_fwd's: entry `name` with `before`, the
    stream and `after`, on device `dev` -- the C side launches on (and sizes
    for) the current device -- and its status raised if nonzero."""
    import torch

    fn = _entry(name)
    st = _raw_stream(stream, dev)
    if dev == torch._C._cuda_getDevice():
        rc = fn(*before, st, *after)
    else:
        with torch.cuda.device(dev):
            rc = fn(*before, st, *after)
    _check(rc)


def _check_qkvo(q, k, v, out):
    """Raise FlashAttentionError unless q, k, v, out are contiguous [B,H,S,D]
    device tensors of one 16-bit dtype, shape and device.  The common case is
    one short-circuit expression (a short launch's host cost is mostly this
    wrapper, tools/host_overhead.py); the per-tensor loop names the culprit."""
    global _DTYPES_16
    if not _DTYPES_16:
        import torch

        _DTYPES_16 = (torch.float16, torch.bfloat16)
    dt, sh, dv = q.dtype, q.shape, q.device
    if (q.is_cuda and len(sh) == 4 and dt in _DTYPES_16 and k.dtype is dt and v.dtype is dt
            and out.dtype is dt and k.shape == sh and v.shape == sh and out.shape == sh
            and k.device == dv and v.device == dv and out.device == dv and q.is_contiguous()
            and k.is_contiguous() and v.is_contiguous() and out.is_contiguous()):
        return
    _check_qkvo_each(q, k, v, out)


def _check_qkvo_each(q, k, v, out):
    import torch

    if q.dtype not in (torch.float16, torch.bfloat16):
        raise FlashAttentionError(FA_ERR_BAD_SHAPE, f"q must be float16 or bfloat16, got {q.dtype}")
    for name, t in (("q", q), ("k", k), ("v", v), ("out", out)):
        if t.dtype != q.dtype:
            raise FlashAttentionError(FA_ERR_BAD_SHAPE, f"{name} must be {q.dtype}, got {t.dtype}")
        if not t.is_cuda:
            raise FlashAttentionError(FA_ERR_NULL_POINTER, f"{name} must be a device tensor")
        if not t.is_contiguous():
            raise FlashAttentionError(FA_ERR_BAD_SHAPE, f"{name} must be contiguous (BHSD)")
        if t.dim() != 4 or t.shape != q.shape:
            raise FlashAttentionError(FA_ERR_BAD_SHAPE, f"{name} must be [B,H,S,D] like q")
        if t.device != q.device:
            raise FlashAttentionError(FA_ERR_BAD_SHAPE,
                                      f"{name} is on {t.device}, q on {q.device}: one device only")


_WS_NEED = {}  # (device, B, H, S, D, causal, piece_tiles) -> workspace bytes (fa_fwd_ws_bytes)
_WS_BUF = {}   # (device, stream) -> zero-filled uint8 workspace, kept for the process


def workspace_bytes(batch: int, heads: int, seq_len: int, head_dim: int, causal: bool,
                    device=None, piece_tiles: int = 0) -> int:
    """Workspace the split tier needs for this call on `device` (0: no split);
    piece_tiles as in :func:`flash_attention_fwd`."""
    import torch

    dev = torch.cuda.current_device() if device is None else torch.device(device).index
    key = (dev, batch, heads, seq_len, head_dim, bool(causal), int(piece_tiles))
    n = _WS_NEED.get(key)
    if n is None:
        with torch.cuda.device(dev):
            n = load_library().fa_fwd_ws_bytes(batch, heads, seq_len, head_dim, int(bool(causal)),
                                               int(piece_tiles))
        _WS_NEED[key] = n
    return n


def _workspace(nbytes: int, dev: int, st: int):
    """A zero-filled workspace of >= nbytes for launches on stream `st` of
    device `dev`, from torch's caching allocator, reused by every later launch
    on that stream (each launch leaves it reusable: fa_mi355x.h).  Under HIP
    graph capture a fresh one is captured with its zero fill instead."""
    import torch

    if torch.cuda.is_current_stream_capturing():
        return torch.zeros(nbytes, dtype=torch.uint8, device=dev)
    buf = _WS_BUF.get((dev, st))
    if buf is None or buf.numel() < nbytes:
        if buf is not None:
            torch.cuda.synchronize(dev)  # launches enqueued on the old one are done
        buf = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
        torch.cuda.current_stream(dev).synchronize()  # the fill lands before any stream uses it
        _WS_BUF[(dev, st)] = buf
    return buf


def flash_attention_fwd(q, k, v, causal: bool = False, out=None, config: Optional[int] = None,
                        stream=None, piece_tiles: int = 0):
    """O = softmax(Q K^T / sqrt(D) [+ causal mask]) V for fp16 or bf16 BHSD tensors.

    q, k, v: [batch, heads, seq_len, D] float16 (the reference's type) or
    bfloat16 contiguous device tensors, all of one dtype; D = 128 (the
    reference's head_dim) or 64.
    config: force a tile config id (see :func:`configs`); default = dispatcher,
    which for long causal launches short of the persistent tier splits query
    blocks' key ranges across workgroups through a workspace from torch's
    caching allocator (fa_fwd_*_ws; :func:`workspace_bytes`).
    piece_tiles > 0 (causal, head_dim 128, config None): force that split
    piece length in 64-key tiles.
    Enqueued on ``stream`` (default: torch's current stream); no sync.
    """
    import torch

    if out is None:
        out = torch.empty_like(q)
    _check_qkvo(q, k, v, out)
    b, h, s, d = q.shape
    lib = _lib or load_library()
    bf16 = q.dtype is torch.bfloat16
    dev = q.device.index
    if stream is None:
        st = torch._C._cuda_getCurrentRawStream(dev)
    else:
        st = stream if isinstance(stream, int) else stream.cuda_stream
    args = (q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), b, h, s, d, int(bool(causal)))
    if config is None:
        need = _WS_NEED.get((dev, b, h, s, d, bool(causal), piece_tiles))
        if need is None:
            need = workspace_bytes(b, h, s, d, causal, device=q.device, piece_tiles=piece_tiles)
        if need or piece_tiles:
            fn = lib.fa_fwd_bf16_ws if bf16 else lib.fa_fwd_f16_ws
            args += (int(piece_tiles), _workspace(need, dev, st).data_ptr() if need else None, need)
        else:
            fn = lib.fa_fwd_bf16 if bf16 else lib.fa_fwd_f16
    else:
        fn = lib.fa_fwd_bf16_config if bf16 else lib.fa_fwd_f16_config
        args += (int(config),)
    # the C side launches on (and sizes for) the current device: make it q's
    if dev == torch._C._cuda_getDevice():
        rc = fn(*args, st)
    else:
        with torch.cuda.device(dev):
            rc = fn(*args, st)
    _check(rc)
    return out


_DEC_NEED = {}  # (device, B, Hq, Hkv, Sq, cap, D, num_splits) -> (workspace bytes, pieces)


def decode_num_splits(batch: int, heads_q: int, heads_kv: int, seqlen_q: int, kv_capacity: int,
                      head_dim: int = HEAD_DIM, device=None) -> int:
    """Pieces the decode entry's plan cuts each cache into on `device` (1: no split)."""
    import torch

    dev = torch.cuda.current_device() if device is None else torch.device(device).index
    with torch.cuda.device(dev):
        return load_library().fa_decode_num_splits(batch, heads_q, heads_kv, seqlen_q,
                                                   kv_capacity, head_dim)


def _kv8_caches(q, kname, k, vname, v, k_scale, v_scale) -> bool:
    """True when both caches are torch.float8_e4m3fn (the kv8 entries), False
    when both have q's dtype; FlashAttentionError for every other pairing and
    for scales given beside a 16-bit cache."""
    import torch

    fp8 = torch.float8_e4m3fn
    if k.dtype is fp8 or v.dtype is fp8:
        if k.dtype != v.dtype:
            raise FlashAttentionError(
                FA_ERR_BAD_SHAPE,
                f"{kname} and {vname} must have one dtype, got {k.dtype} and {v.dtype}")
        return True
    other_fp8 = tuple(getattr(torch, n) for n in ("float8_e4m3fnuz", "float8_e5m2", "float8_e5m2fnuz",
                                                  "float8_e8m0fnu") if hasattr(torch, n))
    for name, t in ((kname, k), (vname, v)):
        if t.dtype in other_fp8:
            raise FlashAttentionError(
                FA_ERR_BAD_SHAPE,
                f"{name}: {t.dtype} is not supported, an FP8 cache must be torch.float8_e4m3fn (OCP E4M3)")
        if t.dtype != q.dtype:
            raise FlashAttentionError(FA_ERR_BAD_SHAPE, f"{name} must be {q.dtype}, got {t.dtype}")
    if k_scale is not None or v_scale is not None:
        raise FlashAttentionError(
            FA_ERR_BAD_SHAPE,
            f"k_scale / v_scale go with a torch.float8_e4m3fn cache only, the cache is {k.dtype}")
    return False


def _check_scales_device(q, k_scale, v_scale):
    for name, t in (("k_scale", k_scale), ("v_scale", v_scale)):
        if t is not None and (not t.is_cuda or t.device != q.device):
            raise FlashAttentionError(FA_ERR_NULL_POINTER, f"{name} must be a tensor on {q.device}")


def _check_decode_head(q, kname, k, vname, v, out, k_scale, v_scale, layout):
    """What both decode checks begin with: q's dtype, the cache pairing
    (:func:`_kv8_caches`, whose answer is returned), then dtype, rank and
    contiguity of q, the caches and out in that order, and out's shape.
    `layout` is what the family's rank and contiguity messages end in."""
    import torch

    if q.dtype not in (torch.float16, torch.bfloat16):
        raise FlashAttentionError(FA_ERR_BAD_SHAPE, f"q must be float16 or bfloat16, got {q.dtype}")
    kv8 = _kv8_caches(q, kname, k, vname, v, k_scale, v_scale)
    for name, t in (("q", q), (kname, k), (vname, v), ("out", out)):
        if t.dtype != q.dtype and not (kv8 and t is not out):
            raise FlashAttentionError(FA_ERR_BAD_SHAPE, f"{name} must be {q.dtype}, got {t.dtype}")
        if t.dim() != 4:
            raise FlashAttentionError(FA_ERR_BAD_SHAPE, f"{name} must be 4-D{layout}")
        if not t.is_contiguous():
            raise FlashAttentionError(FA_ERR_BAD_SHAPE, f"{name} must be contiguous{layout}")
    if out.shape != q.shape:
        raise FlashAttentionError(FA_ERR_BAD_SHAPE, "out must be [B,Hq,Sq,D] like q")
    return kv8


def _check_table_type(block_table):
    import torch

    if block_table.dtype != torch.int32:
        raise FlashAttentionError(FA_ERR_BAD_SHAPE,
                                  f"block_table must be int32, got {block_table.dtype}")
    if block_table.dim() != 2:
        raise FlashAttentionError(FA_ERR_BAD_SHAPE, "block_table must be 2-D [B, max_pages_per_seq]")


def _check_decode_tail(q, kname, k, vname, v, out, k_scale, v_scale, block_table, kv_lens,
                       qname="q", oname="out", batch=None, sinks=None, tree_mask=None):
    """What both decode checks end with, after the family's own shape checks:
    Hq % Hkv, each scale (if given) a contiguous float32 [Hkv] tensor, the
    block table (paged only: None otherwise), kv_lens, and then where all of
    them live.  The append checks end with it too, with k_new and v_new
    (`qname`, `oname`) in the places of q and out.  `batch`: the number of
    sequences where q's first extent is not it (the packed wrappers, whose q is
    [T,Hq,D]: heads are extent 1 there too).  `sinks` (the decode and prefill
    wrappers only): a contiguous float32 [Hq] tensor, checked after the scales
    and like them; its values are not looked at.  `tree_mask` (the decode
    wrappers only): :func:`_check_tree_mask`, after kv_lens in both stages."""
    import torch

    if batch is None:
        batch = q.shape[0]
    heads_kv = k.shape[1]
    if heads_kv == 0 or q.shape[1] % heads_kv != 0:
        raise FlashAttentionError(FA_ERR_BAD_SHAPE,
                                  f"heads_q {q.shape[1]} is not a multiple of heads_kv {heads_kv}")
    for name, t in (("k_scale", k_scale), ("v_scale", v_scale)):
        if t is None:
            continue
        if (not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.dim() != 1
                or t.shape[0] != heads_kv or not t.is_contiguous()):
            got = f"{t.dtype} {list(t.shape)}" if isinstance(t, torch.Tensor) else type(t).__name__
            raise FlashAttentionError(
                FA_ERR_BAD_SHAPE,
                f"{name} must be a contiguous float32 [Hkv = {heads_kv}] tensor, got {got}")
    if sinks is not None:
        t = sinks
        if (not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.dim() != 1
                or t.shape[0] != q.shape[1] or not t.is_contiguous()):
            got = f"{t.dtype} {list(t.shape)}" if isinstance(t, torch.Tensor) else type(t).__name__
            raise FlashAttentionError(
                FA_ERR_BAD_SHAPE,
                f"sinks must be a contiguous float32 [Hq = {q.shape[1]}] tensor, got {got}")
    if block_table is not None:
        _check_table_type(block_table)
        if block_table.shape[0] != batch:
            raise FlashAttentionError(
                FA_ERR_BAD_SHAPE,
                f"block_table has {block_table.shape[0]} rows, {qname} a batch of {batch}")
        if not block_table.is_contiguous():
            raise FlashAttentionError(FA_ERR_BAD_SHAPE, "block_table must be contiguous")
    if kv_lens is not None:
        if kv_lens.dtype != torch.int32:
            raise FlashAttentionError(FA_ERR_BAD_SHAPE, f"kv_lens must be int32, got {kv_lens.dtype}")
        if kv_lens.dim() != 1 or kv_lens.shape[0] != batch or not kv_lens.is_contiguous():
            raise FlashAttentionError(FA_ERR_BAD_SHAPE, "kv_lens must be a contiguous [B] tensor")
    _check_tree_mask(q, tree_mask, False)
    for name, t in ((qname, q), (kname, k), (vname, v), (oname, out)):
        if not t.is_cuda:
            raise FlashAttentionError(FA_ERR_NULL_POINTER, f"{name} must be a device tensor")
        if t.device != q.device:
            raise FlashAttentionError(
                FA_ERR_BAD_SHAPE, f"{name} is on {t.device}, {qname} on {q.device}: one device only")
    for name, t in (("block_table", block_table), ("kv_lens", kv_lens)):
        if t is not None and (not t.is_cuda or t.device != q.device):
            raise FlashAttentionError(FA_ERR_NULL_POINTER, f"{name} must be a tensor on {q.device}")
    _check_scales_device(q, k_scale, v_scale)
    if sinks is not None and (not sinks.is_cuda or sinks.device != q.device):
        raise FlashAttentionError(FA_ERR_NULL_POINTER, f"sinks must be a tensor on {q.device}")
    _check_tree_mask(q, tree_mask, True)


def _check_q_lens(q, q_lens, where):
    """The prefill wrappers' q_lens, worded like the append wrappers' new_lens:
    dtype and shape (`where` false, before the tensors' devices are looked at),
    then its device (`where` true)."""
    if q_lens is None:
        return
    if where:
        if not q_lens.is_cuda or q_lens.device != q.device:
            raise FlashAttentionError(FA_ERR_NULL_POINTER, f"q_lens must be a tensor on {q.device}")
        return
    import torch

    if q_lens.dtype != torch.int32:
        raise FlashAttentionError(FA_ERR_BAD_SHAPE, f"q_lens must be int32, got {q_lens.dtype}")
    if q_lens.dim() != 1 or q_lens.shape[0] != q.shape[0] or not q_lens.is_contiguous():
        raise FlashAttentionError(FA_ERR_BAD_SHAPE, "q_lens must be a contiguous [B] tensor")


def _check_decode(q, k_cache, v_cache, kv_lens, out, k_scale=None, v_scale=None, q_lens=None, sinks=None,
                  tree_mask=None):
    """Raise FlashAttentionError unless q/out are contiguous [B,Hq,Sq,D] and
    k_cache/v_cache contiguous [B,Hkv,cap,D] device tensors of one 16-bit dtype
    (or both torch.float8_e4m3fn beside a 16-bit q, with optional float32
    [Hkv] scales: returns True then) and device with Hq % Hkv == 0, and
    kv_lens (if given) is int32 [B] there.
    Dtypes, ranks and shapes are checked before where the tensors live, so
    each rejection names its own cause whatever the device.  q_lens (the
    prefill wrappers only): int32 [B], checked like kv_lens.  tree_mask (the
    decode wrappers only): int32 [B, Sq], checked like them, last."""
    kv8 = _check_decode_head(q, "k_cache", k_cache, "v_cache", v_cache, out, k_scale, v_scale, " (BHSD)")
    if k_cache.shape != v_cache.shape:
        raise FlashAttentionError(FA_ERR_BAD_SHAPE, "k_cache and v_cache must have one shape")
    if k_cache.shape[0] != q.shape[0] or k_cache.shape[3] != q.shape[3]:
        raise FlashAttentionError(FA_ERR_BAD_SHAPE, "q and the caches must agree in batch and head_dim")
    _check_q_lens(q, q_lens, False)
    _check_decode_tail(q, "k_cache", k_cache, "v_cache", v_cache, out, k_scale, v_scale, None, kv_lens,
                       sinks=sinks, tree_mask=tree_mask)
    _check_q_lens(q, q_lens, True)
    return kv8


def _check_decode_paged(q, k_pages, v_pages, block_table, kv_lens, out, k_scale=None, v_scale=None,
                        q_lens=None, sinks=None, tree_mask=None):
    """Raise FlashAttentionError unless q/out are contiguous [B,Hq,Sq,D],
    k_pages/v_pages contiguous [num_pages,Hkv,page_size,D] pools of q's 16-bit
    dtype (or both torch.float8_e4m3fn, with optional float32 [Hkv] scales:
    returns True then) with page_size % 64 == 0 and Hq % Hkv == 0, block_table a contiguous
    int32 [B,max_pages] tensor and kv_lens (if given) int32 [B], all on q's
    device.  Dtypes, ranks and shapes are checked before where the tensors
    live, so each rejection names its own cause whatever the device.  The
    table's and the lengths' VALUES are not looked at (no sync)."""
    kv8 = _check_decode_head(q, "k_pages", k_pages, "v_pages", v_pages, out, k_scale, v_scale, "")
    if k_pages.shape != v_pages.shape:
        raise FlashAttentionError(FA_ERR_BAD_SHAPE, "k_pages and v_pages must have one shape")
    if k_pages.shape[3] != q.shape[3]:
        raise FlashAttentionError(FA_ERR_BAD_SHAPE, "q and the page pools must agree in head_dim")
    if k_pages.shape[0] == 0:
        raise FlashAttentionError(FA_ERR_BAD_SHAPE, "the page pools hold no page")
    if k_pages.shape[2] == 0 or k_pages.shape[2] % 64 != 0:
        raise FlashAttentionError(FA_ERR_BAD_SHAPE,
                                  f"page_size {k_pages.shape[2]} is not a positive multiple of 64")
    _check_q_lens(q, q_lens, False)
    _check_decode_tail(q, "k_pages", k_pages, "v_pages", v_pages, out, k_scale, v_scale, block_table,
                       kv_lens, sinks=sinks, tree_mask=tree_mask)
    _check_q_lens(q, q_lens, True)
    return kv8


def _check_window(window, causal) -> int:
    """The sliding window W of the decode / prefill functions: 0 = none, W >= 1
    = a row sees at most W keys, its own included (causal only).  Returns the
    value the C entry takes: a W past INT_MAX is INT_MAX (a C int; the entry
    clamps W to the capacity anyway, past which it masks nothing)."""
    if isinstance(window, bool) or not isinstance(window, int):
        raise FlashAttentionError(FA_ERR_BAD_SHAPE,
                                  f"window must be an int, got {type(window).__name__}")
    if window < 0:
        raise FlashAttentionError(FA_ERR_BAD_SHAPE, f"window must be >= 0 (0: no window), got {window}")
    if window > 0 and not causal:
        raise FlashAttentionError(FA_ERR_BAD_SHAPE, "a window needs causal=True (no look-ahead windows)")
    return min(window, 0x7fffffff)


def decode_window_capacity(kv_capacity: int, seqlen_q: int, window: int) -> int:
    """The capacity a windowed decode plans its split from and sizes its
    workspace for (csrc/fa_decode_host.hpp): the tiles holding the last W + Sq
    - 1 keys, min(cap, 64 * ceil((W + Sq - 1) / 64) + 64); window 0: cap."""
    if window <= 0:
        return kv_capacity
    return min(kv_capacity, 64 * ((window + seqlen_q - 1 + 63) // 64) + 64)


def _entry_variant(window, sinks):
    """Which twin of an entry a call takes and what it passes after `causal`:
    sinks given: the `_sink` entry with (window, sinks), window 0 included;
    else window > 0: the `_win` entry with (window,); else the plain entry."""
    if sinks is not None:
        return "_sink", (window, sinks.data_ptr())
    return ("_win", (window,)) if window else ("", ())


def _check_tree_mask(q, tree_mask, where):
    """The decode wrappers' tree_mask, worded like sinks: a contiguous int32
    [B, Sq] tensor (`where` false, before the tensors' devices are looked at),
    then its device (`where` true).  Its values are not looked at (no sync)."""
    t = tree_mask
    if t is None:
        return
    if where:
        if not t.is_cuda or t.device != q.device:
            raise FlashAttentionError(FA_ERR_NULL_POINTER, f"tree_mask must be a tensor on {q.device}")
        return
    import torch

    if (not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or t.dim() != 2
            or tuple(t.shape) != (q.shape[0], q.shape[2]) or not t.is_contiguous()):
        got = f"{t.dtype} {list(t.shape)}" if isinstance(t, torch.Tensor) else type(t).__name__
        raise FlashAttentionError(
            FA_ERR_BAD_SHAPE,
            f"tree_mask must be a contiguous int32 [B = {q.shape[0]}, Sq = {q.shape[2]}] tensor, got {got}")


def _check_tree_rules(q, causal, window):
    """What the tree entries refuse beyond their `_sink` twins, after the
    tensors: causal=False (the mask replaces the causal rule) and a window
    shorter than the drafts."""
    if not causal:
        raise FlashAttentionError(FA_ERR_BAD_SHAPE,
                                  "tree_mask needs causal=True (the mask replaces the causal rule)")
    if 0 < window < q.shape[2]:
        raise FlashAttentionError(
            FA_ERR_BAD_SHAPE,
            f"with tree_mask a window must be 0 or >= Sq = {q.shape[2]} (every ancestor inside it), got {window}")


def tree_mask_from_parents(parents):
    """The tree_mask of :func:`flash_attention_decode` from parent indices.

    parents: an integer tensor [B, Sq] (Sq <= 16), parents[b, t] < t the draft
    token that token t hangs from, -1 for a child of the cached prefix.
    Returns the int32 [B, Sq] ancestor masks m_t = (1 << t) | m_parent (the
    chain parents[b, t] = t - 1 gives (2 << t) - 1), computed on parents'
    device in ceil(log2(Sq)) rounds of pointer doubling: no loop over tokens,
    no sync, graph-capturable.  The values are not validated: an index outside
    [-1, Sq) is read as the nearest inside it."""
    import torch

    if (not isinstance(parents, torch.Tensor) or parents.dim() != 2 or parents.dtype.is_floating_point
            or parents.dtype in (torch.bool, torch.complex64, torch.complex128) or not 1 <= parents.shape[1] <= 16):
        got = f"{parents.dtype} {list(parents.shape)}" if isinstance(parents, torch.Tensor) else type(parents).__name__
        raise FlashAttentionError(FA_ERR_BAD_SHAPE,
                                  f"parents must be an integer [B, Sq <= 16] tensor, got {got}")
    b, sq = parents.shape
    up = parents.to(torch.int64).clamp(-1, sq - 1)  # the ancestor `span` levels up, -1 past the root
    m = (1 << torch.arange(sq, dtype=torch.int64, device=parents.device)).expand(b, sq)  # levels < span
    span = 1
    while span < sq:
        has, idx = up >= 0, up.clamp(min=0)
        m = m | torch.where(has, m.gather(1, idx), 0)
        up = torch.where(has, up.gather(1, idx), up)
        span *= 2
    return m.to(torch.int32).contiguous()


def _decode_call(kv8, q, k, v, out, block_table, kv_lens, causal, return_lse, num_splits, stream,
                 k_scale, v_scale, window=0, sinks=None, tree_mask=None):
    """The call of both decode functions after their checks: the optional LSE,
    the split plan and its workspace, and the fa_decode* entry.
    block_table: None when k, v are a contiguous cache, the table when they are
    page pools (the _paged entries); kv8: the _kv8 entries, which also take the
    two scales; window > 0: the fa_decode_win_* entries, whose plan and
    workspace follow :func:`decode_window_capacity`; sinks: the
    fa_decode_sink_* entries, at any window; tree_mask: the fa_decode_tree_*
    entries (include/fa_mi355x_tree.h), at any window and sinks."""
    import torch

    variant, win = _entry_variant(window, sinks)  # checked by the public function
    if tree_mask is not None:
        variant, win = "_tree", (window, sinks.data_ptr() if sinks is not None else None, tree_mask.data_ptr())
    b, hq, sq, d = q.shape
    hkv, cap = k.shape[1], k.shape[2]
    paged = block_table is not None
    if paged:
        cap *= block_table.shape[1]
    dev = q.device.index
    st = _raw_stream(stream, dev)
    lse = torch.empty((b, hq, sq), dtype=torch.float32, device=q.device) if return_lse else None
    ns = int(num_splits)
    need = 0
    if not paged or cap <= 0x7fffffff - 64:  # (past it the paged entry itself refuses the shape)
        # a windowed call plans (and needs a workspace) as for the window's capacity
        pcap = decode_window_capacity(cap, sq, window)
        key = (dev, b, hq, hkv, sq, pcap, d, ns)
        need = _DEC_NEED.get(key)
    if need is None or need:
        # on q's device: the plan is the current device's, and _workspace asks
        # whether the current device's stream is capturing
        with torch.cuda.device(dev):
            if need is None:
                need = _DEC_NEED[key] = _entry("fa_decode_ws_bytes")(b, hq, hkv, sq, pcap, d, ns)
            ws = _workspace(need, dev, st) if need else None  # (a tensor: alive until the launch)
    _launch(_entry_name("fa_decode", variant, paged, kv8, q.dtype is torch.bfloat16), dev, st,
            (q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(),
             lse.data_ptr() if return_lse else None, b, hq, hkv, sq, *_cache_args(k, d, block_table),
             kv_lens.data_ptr() if kv_lens is not None else None, int(bool(causal)), *win, ns,
             ws.data_ptr() if need else None, need),
            _scale_args(kv8, k_scale, v_scale))
    return (out, lse) if return_lse else out




def flash_attention_decode(q, k_cache, v_cache, kv_lens=None, causal: bool = True, out=None,
                           return_lse: bool = False, num_splits: int = 0, stream=None,
                           k_scale=None, v_scale=None, window: int = 0, sinks=None, tree_mask=None):
    """Decode attention over a K/V cache (fa_decode_f16 / fa_decode_bf16, or
    fa_decode_kv8_* over an FP8 cache).

    q: [B, Hq, Sq, D] (1 <= Sq <= 16); k_cache, v_cache: [B, Hkv, cap, D] with
    Hq % Hkv == 0 (GQA / MQA); fp16 or bf16 contiguous device tensors of one
    dtype, D = 128 or 64.  kv_lens: int32 [B] on the same device (None: every
    length is cap); rows past a length are never read.  causal: bottom-right
    aligned (query token t sees keys <= len - Sq + t).  num_splits: 0 = the
    plan's choice (:func:`decode_num_splits`), > 0 forces that many key pieces.
    Returns out, or (out, lse) with lse fp32 [B, Hq, Sq] (natural log) when
    return_lse.  Enqueued on ``stream`` (default: torch's current stream); no
    sync, graph-capturable; a split launch takes its workspace from the same
    per-(device, stream) buffer as :func:`flash_attention_fwd`.

    FP8 cache: when k_cache and v_cache are both torch.float8_e4m3fn (q and
    out stay 16-bit), K is read as k_scale[hkv] * k_cache and V as
    v_scale[hkv] * v_cache; k_scale, v_scale: contiguous float32 [Hkv] tensors
    on q's device (None: 1.0).  Their values are read on the device, so a
    captured graph follows them.  Scales beside a 16-bit cache are an error.

    window: 0 = none; W >= 1 = sliding-window attention (causal only): the row
    at position pos sees the keys max(0, pos - W + 1) .. pos, at most W, its
    own included -- Hugging Face's ``sliding_window = W``, flash-attn's
    ``window_size = (W - 1, 0)`` (the fa_decode_win_* entries).  Cache rows below
    the first row's lower bound are never read, and in the paged form neither
    are the table entries of pages lying wholly below it: those pages may be
    freed or reused.
    With num_splits = 0 a windowed call is planned from
    :func:`decode_window_capacity`, the keys it can touch.

    sinks: None, or attention sinks: a contiguous float32 [Hq] tensor on q's
    device, one learned logit per query head that joins the softmax
    denominator and contributes no value (the fa_decode_sink_* entries, at any
    window, 0 included, and with causal=False when window=0).  With s_j the
    row's scaled scores (after 1/sqrt(D) and k_scale) over the keys it sees --
    the same keys as without sinks -- den = exp(sinks[h]) + sum_j exp(s_j),
    out = sum_j exp(s_j) v_j / den and lse = log(den); the sink takes neither
    1/sqrt(D) nor k_scale.  A row that sees no key gives zeros and lse =
    sinks[h]; -inf is "no sink for that head".  The values are read on the
    device, so a captured graph follows them; the split plan and the workspace
    are unchanged.  lse includes the sink: a caller merging partial states by
    their lse must pass sinks to ONE partial only.

    tree_mask: None (exactly the call above), or the tree of a speculative
    decoding step (EAGLE / Medusa style verification; the fa_decode_tree_*
    entries of include/fa_mi355x_tree.h, at the given window and sinks): a
    contiguous int32 [B, Sq] tensor on q's device, shared by the heads.  The Sq
    query tokens are draft tokens whose K/V were appended before the call (the
    last Sq rows below kv_lens); bit i of tree_mask[b, t] says that token t sees
    draft token i -- its ancestors and itself, :func:`tree_mask_from_parents` --
    and every token sees the whole prefix.  With a window, token t's position
    is kv_lens[b] - Sq + depth_t, depth_t = popcount - 1, and a prefix key j is
    seen iff j > position - W; W must be 0 or >= Sq.  causal must be True (the
    mask replaces the causal rule).  The chain mask (2 << t) - 1 gives the call
    without tree_mask bit for bit.  Bits from Sq on are ignored and any contents
    are safe: the mask only deselects keys.  It is read on the device: no sync,
    and a captured graph follows a mask rewritten between replays.  A row that
    sees no key gives zeros and lse = -inf (sinks[h] with sinks).
    """
    window = _check_window(window, causal)  # before the tensors: a bad window is named whatever they are
    if out is None:
        import torch

        out = torch.empty_like(q)
    kv8 = _check_decode(q, k_cache, v_cache, kv_lens, out, k_scale, v_scale, sinks=sinks, tree_mask=tree_mask)
    if tree_mask is not None:
        _check_tree_rules(q, causal, window)
    return _decode_call(kv8, q, k_cache, v_cache, out, None, kv_lens, causal, return_lse, num_splits,
                        stream, k_scale, v_scale, window, sinks, tree_mask)


def flash_attention_decode_paged(q, k_pages, v_pages, block_table, kv_lens=None, causal: bool = True,
                                 out=None, return_lse: bool = False, num_splits: int = 0, stream=None,
                                 k_scale=None, v_scale=None, window: int = 0, sinks=None, tree_mask=None):
    """Decode attention over a paged K/V cache (fa_decode_paged_f16 / _bf16, or
    fa_decode_paged_kv8_* over an FP8 pool).

    q: [B, Hq, Sq, D] (1 <= Sq <= 16); k_pages, v_pages: the page pools,
    [num_pages, Hkv, page_size, D] (BHSD inside a page, the serving stacks'
    "HND" layout) with page_size % 64 == 0 and Hq % Hkv == 0; fp16 or bf16
    contiguous device tensors of one dtype, D = 128 or 64.  block_table: int32
    [B, max_pages_per_seq] on the same device; entry j of row b is the pool
    page holding keys [j * page_size, (j + 1) * page_size) of element b (pages
    may be shared and repeated).  kv_lens: int32 [B] (None: every length is
    max_pages_per_seq * page_size).  Only table entries and rows below a
    length are read; nothing is validated on the host, and a page id outside
    the pool reads as zero rows (include/fa_mi355x.h).  The other arguments,
    the return value and the contract (no sync, graph-capturable, the
    per-(device, stream) workspace) are those of :func:`flash_attention_decode`,
    whose result on the gathered cache this one equals bit for bit.  Pools of
    torch.float8_e4m3fn with k_scale / v_scale, and window: as for that
    function (fa_decode_win_paged_*); block-table entries of pages wholly
    below the window are never read.  sinks: as for that function
    (fa_decode_sink_paged_*): pass them to one partial only when merging by lse.
    tree_mask: as for that function (fa_decode_tree_paged_*).
    """
    window = _check_window(window, causal)  # before the tensors: a bad window is named whatever they are
    if out is None:
        import torch

        out = torch.empty_like(q)
    kv8 = _check_decode_paged(q, k_pages, v_pages, block_table, kv_lens, out, k_scale, v_scale,
                              sinks=sinks, tree_mask=tree_mask)
    if tree_mask is not None:
        _check_tree_rules(q, causal, window)
    return _decode_call(kv8, q, k_pages, v_pages, out, block_table, kv_lens, causal, return_lse,
                        num_splits, stream, k_scale, v_scale, window, sinks, tree_mask)


def _prefill_call(family, kv8, q, k, v, out, batch, seqlen_q, block_table, kv_lens, q_lens, causal,
                  return_lse, stream, k_scale, v_scale, window=0, sinks=None):
    """The call of the four prefill functions after their checks (the twin of
    :func:`_decode_call`, without a workspace): the optional LSE and the entry
    of the cache form and q's dtype.  fa_prefill: q [B,Hq,Sq,D], `batch` B,
    `seqlen_q` Sq; fa_prefill_varlen: q [T,Hq,D], `batch` the sequences,
    `seqlen_q` T and `q_lens` the cu_seqlens_q (the lists are one).  The LSE
    ([B,Hq,Sq] / [Hq,T]) is allocated with empty(): rows past q_lens are not
    written.  window > 0: the _win entries; sinks: the _sink entries, at any
    window."""
    import torch

    variant, win = _entry_variant(window, sinks)  # checked by the public function
    hq = q.shape[1]
    lse = None
    if return_lse:
        lse = torch.empty((batch, hq, seqlen_q) if q.dim() == 4 else (hq, seqlen_q), dtype=torch.float32,
                          device=q.device)
    _launch(_entry_name(family, variant, block_table is not None, kv8, q.dtype is torch.bfloat16),
            q.device.index, stream,
            (q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(),
             lse.data_ptr() if return_lse else None, batch, hq, k.shape[1], seqlen_q,
             *_cache_args(k, q.shape[-1], block_table),
             kv_lens.data_ptr() if kv_lens is not None else None,
             q_lens.data_ptr() if q_lens is not None else None, int(bool(causal)), *win),
            _scale_args(kv8, k_scale, v_scale))
    return (out, lse) if return_lse else out




def flash_attention_prefill(q, k_cache, v_cache, kv_lens=None, q_lens=None, causal: bool = True,
                            out=None, return_lse: bool = False, stream=None, k_scale=None,
                            v_scale=None, window: int = 0, sinks=None):
    """Prefill attention over a K/V cache (fa_prefill_f16 / fa_prefill_bf16, or
    fa_prefill_kv8_* over an FP8 cache): a prompt, or a chunk of one behind a
    cached prefix, against the cache :func:`flash_attention_cache_append` wrote
    and :func:`flash_attention_decode` reads.

    q: [B, Hq, Sq, D] (Sq >= 1, any length); k_cache, v_cache: [B, Hkv, cap, D]
    with Hq % Hkv == 0 (GQA / MQA); fp16 or bf16 contiguous device tensors of
    one dtype (or the caches both torch.float8_e4m3fn, with k_scale / v_scale
    as for decode), D = 128 or 64.  kv_lens: int32 [B], the lengths AFTER the
    chunk was appended (None: cap).  q_lens: int32 [B], the tensor the append
    took as new_lens (None: Sq): element b uses its first n_b = clamp(q_lens[b],
    0, Sq) rows.  causal: bottom-right aligned, row t of element b sees keys
    < kv_lens[b] - n_b + t + 1.  A row that sees no key gives zeros and LSE =
    -inf.  Rows t >= n_b of out and lse are not written: with out=None (an
    empty_like(q)) they are unspecified.  Cache rows past a length are never
    read.  Returns out, or (out, lse) with lse fp32 [B, Hq, Sq] (natural log)
    when return_lse.  Lengths and scales are read on the device: no sync, no
    workspace, graph-capturable; enqueued on ``stream`` (default: torch's
    current stream).

    window: 0 = none; W >= 1 = sliding-window attention (causal only): the row
    at position pos sees the keys max(0, pos - W + 1) .. pos, at most W, its
    own included -- Hugging Face's ``sliding_window = W``, flash-attn's
    ``window_size = (W - 1, 0)`` (the fa_prefill_win_* entries).  Cache rows below
    a 128-row query block's first lower bound are never read, and in the paged form neither
    are the table entries of pages lying wholly below it: those pages may be
    freed or reused.
    pos = kv_lens[b] - n_b + t.

    sinks: None, or attention sinks: a contiguous float32 [Hq] tensor on q's
    device, one learned logit per query head that joins the softmax
    denominator and contributes no value (the fa_prefill_sink_* entries, at
    any window, 0 included, and with causal=False when window=0).  With s_j
    the row's scaled scores (after 1/sqrt(D) and k_scale) over the keys it
    sees -- the same keys as without sinks -- den = exp(sinks[h]) + sum_j
    exp(s_j), out = sum_j exp(s_j) v_j / den and lse = log(den); the sink takes
    neither 1/sqrt(D) nor k_scale.  A row that sees no key gives zeros and lse
    = sinks[h]; -inf is "no sink for that head".  The values are read on the
    device, so a captured graph follows them.  lse includes the sink: a caller
    merging partial states by their lse (chunks of one cache attended
    separately) must pass sinks to ONE partial only.
    """
    window = _check_window(window, causal)  # before the tensors: a bad window is named whatever they are
    if out is None:
        import torch

        out = torch.empty_like(q)
    kv8 = _check_decode(q, k_cache, v_cache, kv_lens, out, k_scale, v_scale, q_lens, sinks)
    return _prefill_call("fa_prefill", kv8, q, k_cache, v_cache, out, q.shape[0], q.shape[2], None, kv_lens,
                         q_lens, causal, return_lse, stream, k_scale, v_scale, window, sinks)


def flash_attention_prefill_paged(q, k_pages, v_pages, block_table, kv_lens=None, q_lens=None,
                                  causal: bool = True, out=None, return_lse: bool = False, stream=None,
                                  k_scale=None, v_scale=None, window: int = 0, sinks=None):
    """:func:`flash_attention_prefill` over the page pools
    :func:`flash_attention_decode_paged` reads (fa_prefill_paged_f16 / _bf16, or
    fa_prefill_paged_kv8_* over an FP8 pool).

    k_pages, v_pages: [num_pages, Hkv, page_size, D] with page_size % 64 == 0;
    block_table: int32 [B, max_pages_per_seq]; kv_lens None: max_pages_per_seq
    * page_size.  Only table entries and rows below a length are read, and a
    page id outside the pool reads as zero rows.  The result equals
    :func:`flash_attention_prefill` on the gathered cache bit for bit.  Rows
    t >= n_b of out and lse are not written (unspecified with out=None).
    window: as for that function (fa_prefill_win_paged_*); block-table entries
    of pages wholly below a query block's window are never read.  sinks: as
    for that function (fa_prefill_sink_paged_*): pass them to one partial only
    when merging by lse.
    """
    window = _check_window(window, causal)  # before the tensors: a bad window is named whatever they are
    if block_table is None:
        raise FlashAttentionError(FA_ERR_NULL_POINTER, "block_table is required")
    if out is None:
        import torch

        out = torch.empty_like(q)
    kv8 = _check_decode_paged(q, k_pages, v_pages, block_table, kv_lens, out, k_scale, v_scale, q_lens,
                              sinks)
    return _prefill_call("fa_prefill", kv8, q, k_pages, v_pages, out, q.shape[0], q.shape[2], block_table,
                         kv_lens, q_lens, causal, return_lse, stream, k_scale, v_scale, window, sinks)


def _check_append(k_new, v_new, kname, k, vname, v, block_table, kv_lens, new_lens, k_scale, v_scale):
    """Raise FlashAttentionError unless k_new / v_new are contiguous
    [B,Hkv,Sn,D] tensors of one 16-bit dtype and shape, the caches (`kname`,
    `vname`: [B,Hkv,cap,D], or with a block table the pools
    [num_pages,Hkv,page_size,D]) have that dtype or are both
    torch.float8_e4m3fn (returns True then) and agree with k_new in Hkv and D
    (and B when contiguous), kv_lens is given, and lengths, table and scales
    are what the decode wrappers take -- in their order and with their
    messages (:func:`_kv8_caches`, :func:`_check_decode_tail`)."""
    import torch

    paged = block_table is not None
    if k_new.dtype not in (torch.float16, torch.bfloat16):
        raise FlashAttentionError(FA_ERR_BAD_SHAPE,
                                  f"k_new must be float16 or bfloat16, got {k_new.dtype}")
    kv8 = _kv8_caches(k_new, kname, k, vname, v, k_scale, v_scale)
    layout = "" if paged else " (BHSD)"
    for name, t in (("k_new", k_new), ("v_new", v_new), (kname, k), (vname, v)):
        if t.dtype != k_new.dtype and not (kv8 and t is not v_new):
            raise FlashAttentionError(FA_ERR_BAD_SHAPE, f"{name} must be {k_new.dtype}, got {t.dtype}")
        if t.dim() != 4:
            raise FlashAttentionError(FA_ERR_BAD_SHAPE, f"{name} must be 4-D{layout}")
        if not t.is_contiguous():
            raise FlashAttentionError(FA_ERR_BAD_SHAPE, f"{name} must be contiguous{layout}")
    if v_new.shape != k_new.shape:
        raise FlashAttentionError(FA_ERR_BAD_SHAPE, "k_new and v_new must have one shape, [B,Hkv,Sn,D]")
    if k_new.shape[2] < 1:
        raise FlashAttentionError(FA_ERR_BAD_SHAPE, "k_new holds no token (Sn must be >= 1)")
    if k.shape != v.shape:
        raise FlashAttentionError(FA_ERR_BAD_SHAPE, f"{kname} and {vname} must have one shape")
    if k.shape[1] != k_new.shape[1] or k.shape[3] != k_new.shape[3]:
        raise FlashAttentionError(
            FA_ERR_BAD_SHAPE,
            f"k_new and the {'page pools' if paged else 'caches'} must agree in heads_kv and head_dim")
    if paged:
        if k.shape[0] == 0:
            raise FlashAttentionError(FA_ERR_BAD_SHAPE, "the page pools hold no page")
        if k.shape[2] == 0 or k.shape[2] % 64 != 0:
            raise FlashAttentionError(FA_ERR_BAD_SHAPE,
                                      f"page_size {k.shape[2]} is not a positive multiple of 64")
    elif k.shape[0] != k_new.shape[0]:
        raise FlashAttentionError(FA_ERR_BAD_SHAPE, "k_new and the caches must agree in batch")
    if kv_lens is None:
        raise FlashAttentionError(
            FA_ERR_NULL_POINTER,
            "kv_lens is required: the int32 [B] lengths after the append (what decode takes next)")
    if new_lens is not None:
        if new_lens.dtype != torch.int32:
            raise FlashAttentionError(FA_ERR_BAD_SHAPE, f"new_lens must be int32, got {new_lens.dtype}")
        if new_lens.dim() != 1 or new_lens.shape[0] != k_new.shape[0] or not new_lens.is_contiguous():
            raise FlashAttentionError(FA_ERR_BAD_SHAPE, "new_lens must be a contiguous [B] tensor")
    _check_decode_tail(k_new, kname, k, vname, v, v_new, k_scale, v_scale, block_table, kv_lens,
                       qname="k_new", oname="v_new")
    if new_lens is not None and (not new_lens.is_cuda or new_lens.device != k_new.device):
        raise FlashAttentionError(FA_ERR_NULL_POINTER, f"new_lens must be a tensor on {k_new.device}")
    return kv8


def _append_call(family, kv8, k_new, v_new, k, v, batch, seqlen_new, block_table, kv_lens, new_lens, stream,
                 k_scale, v_scale, rope=()):
    """The call of the eight append functions after their checks: the entry of
    the cache form.  fa_cache_append / fa_rope_append: k_new [B,Hkv,Sn,D],
    `batch` B, `seqlen_new` Sn; their _varlen twins: k_new [T,Hkv,D], `batch`
    the sequences, `seqlen_new` T and `new_lens` the cu_seqlens (the lists are
    one).  rope: the fa_rope_append* entries' :func:`_rope_tail`."""
    import torch

    _launch(_entry_name(family, "", block_table is not None, kv8, k_new.dtype is torch.bfloat16),
            k_new.device.index, stream,
            (k_new.data_ptr(), v_new.data_ptr(), k.data_ptr(), v.data_ptr(), batch, k_new.shape[1],
             seqlen_new, *_cache_args(k, k_new.shape[-1], block_table), kv_lens.data_ptr(),
             new_lens.data_ptr() if new_lens is not None else None),
            _scale_args(kv8, k_scale, v_scale) + rope)




def flash_attention_cache_append(k_new, v_new, k_cache, v_cache, kv_lens, new_lens=None,
                                 k_scale=None, v_scale=None, stream=None) -> None:
    """Write new K/V tokens into the cache :func:`flash_attention_decode`
    reads (fa_cache_append_16, or fa_cache_append_kv8_* into an FP8 cache), K
    and V in one launch.

    k_new, v_new: [B, Hkv, Sn, D] fp16 or bf16 contiguous device tensors of one
    shape (Sn >= 1, D = 128 or 64); k_cache, v_cache: [B, Hkv, cap, D],
    contiguous, of k_new's dtype or both torch.float8_e4m3fn.  kv_lens: int32
    [B], REQUIRED: the lengths AFTER the append, the tensor the following
    decode call takes.  new_lens: int32 [B] (None: Sn everywhere); element b
    appends its first n_b = clamp(new_lens[b], 0, Sn) tokens, token t to cache
    row kv_lens[b] - n_b + t.  A row is written iff it lies in [0, cap)
    (kv_lens is not clamped); nothing else in the caches is touched.

    FP8 cache: the stored byte is E4M3(clamp(float(x) * (1.0f / s), -448,
    448)), round to nearest even, with s = k_scale[hkv] / v_scale[hkv]
    (float32 [Hkv] device tensors, None: 1.0) -- the reciprocal-multiply form
    is the contract (include/fa_mi355x.h).  Scales beside a 16-bit cache are an
    error.  Lengths and scales are read on the device: no sync, no workspace,
    graph-capturable.  Returns None.
    """
    kv8 = _check_append(k_new, v_new, "k_cache", k_cache, "v_cache", v_cache, None, kv_lens, new_lens,
                        k_scale, v_scale)
    _append_call("fa_cache_append", kv8, k_new, v_new, k_cache, v_cache, k_new.shape[0], k_new.shape[2], None,
                 kv_lens, new_lens, stream, k_scale, v_scale)


def flash_attention_cache_append_paged(k_new, v_new, k_pages, v_pages, block_table, kv_lens,
                                       new_lens=None, k_scale=None, v_scale=None, stream=None) -> None:
    """:func:`flash_attention_cache_append` into the page pools
    :func:`flash_attention_decode_paged` reads (fa_cache_append_paged_16 /
    fa_cache_append_paged_kv8_*).

    k_pages, v_pages: [num_pages, Hkv, page_size, D] with page_size % 64 == 0;
    block_table: int32 [B, max_pages_per_seq].  Row r of element b lives in
    page block_table[b, r // page_size] at offset r % page_size and is written
    iff r lies in [0, max_pages_per_seq * page_size) and that id in [0,
    num_pages): an out-of-pool id drops the row (the write-side twin of "reads
    as zero rows").  Two elements whose tables map the same page row race: one
    wins, unspecified which.  Everything else as for the contiguous function;
    the table is read on the device.  Returns None.
    """
    if block_table is None:
        raise FlashAttentionError(FA_ERR_NULL_POINTER, "block_table is required")
    kv8 = _check_append(k_new, v_new, "k_pages", k_pages, "v_pages", v_pages, block_table, kv_lens,
                        new_lens, k_scale, v_scale)
    _append_call("fa_cache_append", kv8, k_new, v_new, k_pages, v_pages, k_new.shape[0], k_new.shape[2],
                 block_table, kv_lens, new_lens, stream, k_scale, v_scale)


def _check_cu_seqlens(cu, name, nseq, ref, where):
    """The packed wrappers' cu_seqlens, worded like q_lens / new_lens: presence,
    dtype and shape (`where` false, before the tensors' devices are looked at),
    then its device (`where` true).  Its VALUES are not looked at (no sync)."""
    if where:
        if not cu.is_cuda or cu.device != ref.device:
            raise FlashAttentionError(FA_ERR_NULL_POINTER, f"{name} must be a tensor on {ref.device}")
        return
    import torch

    if cu is None:
        raise FlashAttentionError(
            FA_ERR_NULL_POINTER,
            f"{name} is required: the int32 [B + 1] prefix sum of the sequences' token counts")
    if cu.dtype != torch.int32:
        raise FlashAttentionError(FA_ERR_BAD_SHAPE, f"{name} must be int32, got {cu.dtype}")
    if cu.dim() != 1 or cu.shape[0] != nseq + 1 or not cu.is_contiguous():
        raise FlashAttentionError(
            FA_ERR_BAD_SHAPE,
            f"{name} must be a contiguous [B + 1 = {nseq + 1}] tensor, got {list(cu.shape)}")


def _check_packed(x, xname, y, yname, kname, k, vname, v, block_table, cu, cuname, kv_lens, k_scale,
                  v_scale, need_kv_lens, sinks=None):
    """What the four packed wrappers check.  x, y: q and out [T,Hq,D] (prefill)
    or k_new and v_new [T,Hkv,D] (append), contiguous, of one 16-bit dtype and
    shape; the caches (`kname`, `vname`: [B,Hkv,cap,D], or with a block table
    the pools [num_pages,Hkv,page_size,D]) of that dtype or both
    torch.float8_e4m3fn (returns True then); B is the caches' batch, or the
    table's rows; cu int32 [B + 1]; the rest as :func:`_check_decode_tail`
    takes it.  Dtypes, ranks and shapes come before where the tensors live."""
    import torch

    paged = block_table is not None
    if x.dtype not in (torch.float16, torch.bfloat16):
        raise FlashAttentionError(FA_ERR_BAD_SHAPE,
                                  f"{xname} must be float16 or bfloat16, got {x.dtype}")
    kv8 = _kv8_caches(x, kname, k, vname, v, k_scale, v_scale)
    for name, t, rank, layout in ((xname, x, 3, " [T,H,D]"), (yname, y, 3, " [T,H,D]"),
                                  (kname, k, 4, "" if paged else " (BHSD)"),
                                  (vname, v, 4, "" if paged else " (BHSD)")):
        if t.dtype != x.dtype and not (kv8 and rank == 4):
            raise FlashAttentionError(FA_ERR_BAD_SHAPE, f"{name} must be {x.dtype}, got {t.dtype}")
        if t.dim() != rank:
            raise FlashAttentionError(FA_ERR_BAD_SHAPE, f"{name} must be {rank}-D{layout}")
        if not t.is_contiguous():
            raise FlashAttentionError(FA_ERR_BAD_SHAPE, f"{name} must be contiguous{layout}")
    if y.shape != x.shape:
        raise FlashAttentionError(FA_ERR_BAD_SHAPE, f"{yname} must be [T,H,D] like {xname}")
    if k.shape != v.shape:
        raise FlashAttentionError(FA_ERR_BAD_SHAPE, f"{kname} and {vname} must have one shape")
    if k.shape[3] != x.shape[2]:
        raise FlashAttentionError(
            FA_ERR_BAD_SHAPE,
            f"{xname} and the {'page pools' if paged else 'caches'} must agree in head_dim")
    if need_kv_lens and k.shape[1] != x.shape[1]:
        raise FlashAttentionError(
            FA_ERR_BAD_SHAPE,
            f"{xname} and the {'page pools' if paged else 'caches'} must agree in heads_kv")
    if paged:
        if k.shape[0] == 0:
            raise FlashAttentionError(FA_ERR_BAD_SHAPE, "the page pools hold no page")
        if k.shape[2] == 0 or k.shape[2] % 64 != 0:
            raise FlashAttentionError(FA_ERR_BAD_SHAPE,
                                      f"page_size {k.shape[2]} is not a positive multiple of 64")
        _check_table_type(block_table)
        nseq = block_table.shape[0]
    else:
        nseq = k.shape[0]
    if need_kv_lens and kv_lens is None:
        raise FlashAttentionError(
            FA_ERR_NULL_POINTER,
            "kv_lens is required: the int32 [B] lengths after the append (what decode takes next)")
    _check_cu_seqlens(cu, cuname, nseq, x, False)
    _check_decode_tail(x, kname, k, vname, v, y, k_scale, v_scale, block_table, kv_lens,
                       qname=xname, oname=yname, batch=nseq, sinks=sinks)
    _check_cu_seqlens(cu, cuname, nseq, x, True)
    return kv8, nseq


def _prefill_varlen(q, k, v, block_table, names, cu_seqlens_q, kv_lens, causal, out, return_lse, stream,
                    k_scale, v_scale, window=0, sinks=None):
    if out is None:
        import torch

        out = torch.empty_like(q)
    kv8, nseq = _check_packed(q, "q", out, "out", names[0], k, names[1], v, block_table, cu_seqlens_q,
                              "cu_seqlens_q", kv_lens, k_scale, v_scale, False, sinks)
    return _prefill_call("fa_prefill_varlen", kv8, q, k, v, out, nseq, q.shape[0], block_table, kv_lens,
                         cu_seqlens_q, causal, return_lse, stream, k_scale, v_scale, window, sinks)

def flash_attention_prefill_varlen(q, k_cache, v_cache, cu_seqlens_q, kv_lens=None, causal: bool = True,
                                   out=None, return_lse: bool = False, stream=None, k_scale=None,
                                   v_scale=None, window: int = 0, sinks=None):
    """:func:`flash_attention_prefill` for a packed ragged batch
    (fa_prefill_varlen_f16 / _bf16, or fa_prefill_varlen_kv8_* over an FP8
    cache): what a serving stack holds after its QKV projection, taken as it
    is, with no padded copy.

    q: [T, Hq, D], token-major, contiguous: the B sequences' query tokens one
    after another.  cu_seqlens_q: int32 [B + 1] on q's device, REQUIRED, the
    prefix sum of the token counts: sequence b is rows [s_b, e_b) with s_b =
    clamp(cu[b], 0, T), e_b = clamp(cu[b + 1], s_b, T), n_b = e_b - s_b.  B is
    the caches' batch.  k_cache, v_cache, kv_lens (the lengths AFTER the chunk
    was appended), causal, the scales: as for :func:`flash_attention_prefill`,
    with n_b in q_lens' place.  Row s_b + t of the result equals row t of
    element b of that function on the padded copy BIT FOR BIT.  Rows that
    belong to no sequence (below cu[0], at or past cu[B]) are not written:
    unspecified with out=None.  Any contents of cu_seqlens_q are memory-safe
    (the clamps); if they do not increase the result is unspecified.  Returns
    out [T, Hq, D], or (out, lse) with lse fp32 [Hq, T] when return_lse.
    Everything is read on the device: no sync, no workspace, graph-capturable.
    window: the sliding window of :func:`flash_attention_prefill`
    (fa_prefill_varlen_win_*), with the same bit-for-bit equality.  sinks: the
    attention sinks of :func:`flash_attention_prefill` (fa_prefill_varlen_sink_*),
    float32 [Hq], with the same equality; pass them to one partial only when
    merging by lse.
    """
    window = _check_window(window, causal)  # before the tensors: a bad window is named whatever they are
    return _prefill_varlen(q, k_cache, v_cache, None, ("k_cache", "v_cache"), cu_seqlens_q, kv_lens,
                           causal, out, return_lse, stream, k_scale, v_scale, window, sinks)


def flash_attention_prefill_varlen_paged(q, k_pages, v_pages, block_table, cu_seqlens_q, kv_lens=None,
                                         causal: bool = True, out=None, return_lse: bool = False,
                                         stream=None, k_scale=None, v_scale=None, window: int = 0, sinks=None):
    """:func:`flash_attention_prefill_varlen` over the page pools of
    :func:`flash_attention_prefill_paged` (fa_prefill_varlen_paged_f16 / _bf16,
    or fa_prefill_varlen_paged_kv8_*).  B is the block table's row count; the
    result equals the contiguous function's on the gathered cache bit for bit.
    window: the sliding window of :func:`flash_attention_prefill`
    (fa_prefill_varlen_win_paged_*); block-table entries of pages wholly below
    a query block's window are never read.  sinks: as for that function
    (fa_prefill_varlen_sink_paged_*): pass them to one partial only when merging
    by lse.
    """
    window = _check_window(window, causal)  # before the tensors: a bad window is named whatever they are
    if block_table is None:
        raise FlashAttentionError(FA_ERR_NULL_POINTER, "block_table is required")
    return _prefill_varlen(q, k_pages, v_pages, block_table, ("k_pages", "v_pages"), cu_seqlens_q,
                           kv_lens, causal, out, return_lse, stream, k_scale, v_scale, window, sinks)


def _token_stride(t, name, rank):
    """The token stride (elements; 0: dense) of a token-major view, [T,H,D] or
    [B,S,H,D]: the last dimension contiguous, heads D apart, and (rank 4) the
    batch stride S token strides, so that tokens are one stride apart
    throughout.  Extents of 1 have no stride to check.  Nothing is copied:
    anything else raises."""
    h, d = t.shape[-2], t.shape[-1]
    if (d > 1 and t.stride(-1) != 1) or (h > 1 and t.stride(-2) != d):
        raise FlashAttentionError(
            FA_ERR_BAD_SHAPE,
            f"{name} must have stride(-1) == 1 and stride(-2) == head_dim (a token-major view; it is "
            f"not copied), got strides {tuple(t.stride())}")
    ntok = t.shape[-3]
    if rank == 4 and t.shape[0] > 1:
        if ntok > 1 and t.stride(0) != ntok * t.stride(1):
            raise FlashAttentionError(
                FA_ERR_BAD_SHAPE,
                f"{name}: the batch stride {t.stride(0)} is not seqlen * the token stride "
                f"{t.stride(1)} (it is not copied)")
        st = t.stride(1) if ntok > 1 else t.stride(0)
    else:
        st = t.stride(-3) if ntok > 1 else 0
    if st % 8 != 0 or (st and st < h * d):
        raise FlashAttentionError(
            FA_ERR_BAD_SHAPE,
            f"{name}: the token stride {st} must be a multiple of 8 elements, at least heads * head_dim")
    return st


def _check_attn(q, k, v, out, rank, cu_q, cu_k, sinks):
    """What flash_attention_varlen (rank 3, [T,H,D]) and flash_attention_bshd
    (rank 4, [B,S,H,D]) check: dtypes, ranks and shapes, then where the tensors
    live, never values.  Returns the three token strides."""
    import torch

    layout = " [T,H,D]" if rank == 3 else " [B,S,H,D]"
    if q.dtype not in (torch.float16, torch.bfloat16):
        raise FlashAttentionError(FA_ERR_BAD_SHAPE, f"q must be float16 or bfloat16, got {q.dtype}")
    for name, t in (("q", q), ("k", k), ("v", v), ("out", out)):
        if t.dtype != q.dtype:
            raise FlashAttentionError(FA_ERR_BAD_SHAPE, f"{name} must be {q.dtype}, got {t.dtype}")
        if t.dim() != rank:
            raise FlashAttentionError(FA_ERR_BAD_SHAPE, f"{name} must be {rank}-D{layout}")
    if not out.is_contiguous():
        raise FlashAttentionError(FA_ERR_BAD_SHAPE, f"out must be contiguous{layout}")
    if out.shape != q.shape:
        raise FlashAttentionError(FA_ERR_BAD_SHAPE, f"out must be{layout} like q")
    if k.shape != v.shape:
        raise FlashAttentionError(FA_ERR_BAD_SHAPE, "k and v must have one shape")
    if k.shape[-1] != q.shape[-1] or (rank == 4 and k.shape[0] != q.shape[0]):
        raise FlashAttentionError(FA_ERR_BAD_SHAPE,
                                  "q, k and v must agree in head_dim" + (" and batch" if rank == 4 else ""))
    strides = tuple(_token_stride(t, name, rank) for name, t in (("q", q), ("k", k), ("v", v)))
    hq, hkv = q.shape[-2], k.shape[-2]
    if hkv == 0 or hq % hkv != 0:
        raise FlashAttentionError(FA_ERR_BAD_SHAPE, f"heads_q {hq} is not a multiple of heads_kv {hkv}")
    if sinks is not None:
        t = sinks
        if (not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.dim() != 1
                or t.shape[0] != hq or not t.is_contiguous()):
            got = f"{t.dtype} {list(t.shape)}" if isinstance(t, torch.Tensor) else type(t).__name__
            raise FlashAttentionError(
                FA_ERR_BAD_SHAPE, f"sinks must be a contiguous float32 [Hq = {hq}] tensor, got {got}")
    if rank == 3:
        if cu_q is None:
            _check_cu_seqlens(None, "cu_seqlens_q", 0, q, False)
        if cu_q.dim() != 1 or cu_q.shape[0] < 1:
            raise FlashAttentionError(FA_ERR_BAD_SHAPE, "cu_seqlens_q must be a [B + 1] tensor")
        nseq = cu_q.shape[0] - 1
        _check_cu_seqlens(cu_q, "cu_seqlens_q", nseq, q, False)
        if cu_k is not None:
            _check_cu_seqlens(cu_k, "cu_seqlens_k", nseq, q, False)
    for name, t in (("q", q), ("k", k), ("v", v), ("out", out)):
        if not t.is_cuda:
            raise FlashAttentionError(FA_ERR_NULL_POINTER, f"{name} must be a device tensor")
        if t.device != q.device:
            raise FlashAttentionError(FA_ERR_BAD_SHAPE,
                                      f"{name} is on {t.device}, q on {q.device}: one device only")
    if rank == 3:
        _check_cu_seqlens(cu_q, "cu_seqlens_q", nseq, q, True)
        if cu_k is not None:
            _check_cu_seqlens(cu_k, "cu_seqlens_k", nseq, q, True)
    if sinks is not None and (not sinks.is_cuda or sinks.device != q.device):
        raise FlashAttentionError(FA_ERR_NULL_POINTER, f"sinks must be a tensor on {q.device}")
    return strides


def _attn_call(q, k, v, out, strides, batch, total_q, total_k, cu_q, cu_k, seqlen_q, seqlen_k, causal,
               lse, stream, window, sinks):
    """The call of the two functions below after their checks: the
    fa_attn_varlen[_win|_sink]_* entry of q's dtype."""
    import torch

    variant, win = _entry_variant(window, sinks)  # window: checked by the public function
    _launch(_entry_name("fa_attn_varlen", variant, False, False, q.dtype is torch.bfloat16),
            q.device.index, stream,
            (q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(),
             lse.data_ptr() if lse is not None else None, batch, q.shape[-2], k.shape[-2], total_q,
             total_k, q.shape[-1], *strides, cu_q.data_ptr() if cu_q is not None else None,
             cu_k.data_ptr() if cu_k is not None else None, seqlen_q, seqlen_k, int(bool(causal)),
             *win[:1]),
            win[1:])  # these entries take `sinks` after the stream


def flash_attention_varlen(q, k, v, cu_seqlens_q, cu_seqlens_k=None, causal: bool = False, out=None,
                           return_lse: bool = False, stream=None, window: int = 0, sinks=None):
    """Attention over token-major Q, K and V with no cache (fa_attn_varlen_f16 /
    _bf16; flash-attn's ``flash_attn_varlen_func``): a packed ragged batch as
    the QKV projection leaves it -- an encoder, a vision tower (causal=False),
    an embedding model, a first prefill whose keys are not cached yet.

    q: [T_q, Hq, D]; k, v: [T_k, Hkv, D] with Hq % Hkv == 0 (GQA / MQA); fp16 or
    bf16 device tensors of one dtype, D = 128 or 64.  Each may be a VIEW with
    stride(-1) == 1 and stride(-2) == D whose token stride is a multiple of 8
    elements -- the three slices of one fused QKV buffer are read in place;
    anything else raises (nothing is ever copied).  cu_seqlens_q, cu_seqlens_k:
    int32 [B + 1] on q's device, read and clamped there as
    :func:`flash_attention_prefill_varlen` reads cu_seqlens_q: sequence b's
    queries are rows [sq_b, sq_b + nq_b) of q and its keys rows [sk_b, sk_b +
    nk_b) of k and v.  cu_seqlens_k=None: self-attention, the keys' spans are
    the queries'.  causal: bottom-right aligned, row t of b sees keys < nk_b -
    nq_b + t + 1 of b.  A row that sees no key gives zeros and LSE = -inf.
    Rows that belong to no sequence are not written (unspecified with
    out=None) and K/V rows that belong to none are never read.  The result
    equals :func:`flash_attention_prefill_varlen` on a contiguous cache holding
    the same keys (kv_lens = nk) BIT FOR BIT.  Any contents of the cu arrays
    are memory-safe.  out: a contiguous [T_q, Hq, D] tensor that does not
    overlap q.  Returns out, or (out, lse) with lse fp32 [Hq, T_q] (natural
    log) when return_lse.  No sync, no workspace, graph-capturable.
    window, sinks: as for :func:`flash_attention_prefill`
    (fa_attn_varlen_win_* / fa_attn_varlen_sink_*), pos = nk_b - nq_b + t.
    """
    window = _check_window(window, causal)  # before the tensors: a bad window is named whatever they are
    import torch

    if out is None:
        out = torch.empty(q.shape, dtype=q.dtype, device=q.device)
    strides = _check_attn(q, k, v, out, 3, cu_seqlens_q, cu_seqlens_k, sinks)
    total_q, hq = q.shape[0], q.shape[1]
    lse = torch.empty((hq, total_q), dtype=torch.float32, device=q.device) if return_lse else None
    _attn_call(q, k, v, out, strides, cu_seqlens_q.shape[0] - 1, total_q, k.shape[0], cu_seqlens_q,
               cu_seqlens_k, 0, 0, causal, lse, stream, window, sinks)
    return (out, lse) if return_lse else out


def flash_attention_bshd(q, k, v, causal: bool = False, out=None, return_lse: bool = False, stream=None,
                         window: int = 0, sinks=None):
    """:func:`flash_attention_varlen` for uniform lengths (flash-attn's
    ``flash_attn_func``): q [B, Sq, Hq, D], k and v [B, Sk, Hkv, D], taken as
    they are -- the entries' uniform mode, with no cu_seqlens tensor and no
    extra launch.  Views as for that function, with stride(0) == S * stride(1)
    (a [B, S, (Hq + 2 Hkv) D] projection output sliced along its last
    dimension qualifies).  causal: bottom-right aligned (row t sees keys < Sk -
    Sq + t + 1).  Returns out [B, Sq, Hq, D] (contiguous), or (out, lse) with
    lse a [B, Hq, Sq] VIEW of the fp32 [Hq, B * Sq] result when return_lse.
    window, sinks: as for that function."""
    window = _check_window(window, causal)  # before the tensors: a bad window is named whatever they are
    import torch

    if out is None:
        out = torch.empty(q.shape, dtype=q.dtype, device=q.device)
    strides = _check_attn(q, k, v, out, 4, None, None, sinks)
    b, sq, hq, _ = q.shape
    sk = k.shape[1]
    lse = torch.empty((hq, b * sq), dtype=torch.float32, device=q.device) if return_lse else None
    _attn_call(q, k, v, out, strides, b, b * sq, b * sk, None, None, sq, sk, causal, lse, stream, window,
               sinks)
    return (out, lse.view(hq, b, sq).permute(1, 0, 2)) if return_lse else out


def _check_attn_bwd(dout, q, k, v, out, lse, rank, cu_q, cu_k, dq, dk, dv, sinks=None, dsinks=None):
    """What the two backward functions check on top of _check_attn (which sees
    q, k, v, the forward's out and its sinks): dout under q's stride rule, the
    LSE's layout, and the gradients (allocated when None; dsinks only with
    sinks).  Returns the four token strides (dout's first), [dq, dk, dv] and
    dsinks (None without sinks)."""
    import torch

    # dout, lse and the gradients before _check_attn, whose last checks are where
    # the tensors live: shapes and layouts are refused whatever the device (a
    # malformed q is _check_attn's to name)
    grads, do_stride = [], 0
    if q.dim() == rank and q.dtype in (torch.float16, torch.bfloat16):
        layout = "[T,H,D]" if rank == 3 else "[B,S,H,D]"
        if dout.dtype != q.dtype or dout.dim() != rank or dout.shape != q.shape:
            raise FlashAttentionError(FA_ERR_BAD_SHAPE, f"dout must be a {q.dtype} {layout} tensor like q")
        do_stride = _token_stride(dout, "dout", rank)
        hq = q.shape[-2]
        if not isinstance(lse, torch.Tensor) or lse.dtype != torch.float32:
            raise FlashAttentionError(FA_ERR_BAD_SHAPE, "lse must be the forward's float32 lse")
        if rank == 3:
            want, want_st = (hq, q.shape[0]), (q.shape[0], 1)
        else:
            b, sq = q.shape[0], q.shape[1]
            want, want_st = (b, hq, sq), (sq, b * sq, 1)
        if tuple(lse.shape) != want or (lse.numel() > 0 and any(
                n > 1 and st != w for n, st, w in zip(want, lse.stride(), want_st))):
            raise FlashAttentionError(
                FA_ERR_BAD_SHAPE,
                "lse must be the forward's lse: " + ("a contiguous [Hq, T_q] tensor" if rank == 3 else
                                                     "the [B, Hq, Sq] view of a [Hq, B * Sq] buffer")
                + f", got {list(lse.shape)} with strides {tuple(lse.stride())}")
        grads = []
        for name, t, like in (("dq", dq, q), ("dk", dk, k), ("dv", dv, v)):
            if t is None:
                t = torch.empty(like.shape, dtype=q.dtype, device=q.device)
            elif t.dtype != q.dtype or t.shape != like.shape or not t.is_contiguous():
                raise FlashAttentionError(FA_ERR_BAD_SHAPE,
                                          f"{name} must be a contiguous {q.dtype} tensor shaped like {name[1]}")
            grads.append(t)
        if sinks is None and dsinks is not None:
            raise FlashAttentionError(FA_ERR_BAD_SHAPE, "dsinks is the gradient of sinks: it needs sinks")
        if sinks is not None and dsinks is not None and (
                not isinstance(dsinks, torch.Tensor) or dsinks.dtype != torch.float32 or dsinks.dim() != 1
                or dsinks.shape[0] != hq or not dsinks.is_contiguous()):
            raise FlashAttentionError(FA_ERR_BAD_SHAPE, f"dsinks must be a contiguous float32 [Hq = {hq}] tensor")
    strides = _check_attn(q, k, v, out, rank, cu_q, cu_k, sinks)
    if sinks is not None and dsinks is None:
        dsinks = torch.empty(sinks.shape, dtype=torch.float32, device=q.device)
    named = [("dout", dout), ("lse", lse), ("dq", grads[0]), ("dk", grads[1]), ("dv", grads[2])]
    for name, t in named + ([("dsinks", dsinks)] if dsinks is not None else []):
        if not t.is_cuda:
            raise FlashAttentionError(FA_ERR_NULL_POINTER, f"{name} must be a device tensor")
        if t.device != q.device:
            raise FlashAttentionError(FA_ERR_BAD_SHAPE,
                                      f"{name} is on {t.device}, q on {q.device}: one device only")
    return (do_stride,) + strides, grads, dsinks


def _attn_bwd_call(dout, q, k, v, out, lse, grads, strides, batch, total_q, total_k, cu_q, cu_k, seqlen_q,
                   seqlen_k, causal, stream, window=0, sinks=None, dsinks=None):
    """The call of the two functions below after their checks: delta (the only
    workspace) and the entry of q's dtype: fa_attn_varlen_bwd_*, or with a
    window fa_attn_bwd_win_*, or with sinks fa_attn_bwd_sink_*."""
    import torch

    variant, win = _entry_variant(window, sinks)  # window: checked by the public function
    delta = torch.empty((q.shape[-2], total_q), dtype=torch.float32, device=q.device)
    dq, dk, dv = grads
    _launch(_entry_name("fa_attn_bwd" if variant else "fa_attn_varlen_bwd", variant, False, False,
                        q.dtype is torch.bfloat16),
            q.device.index, stream,
            (dout.data_ptr(), q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), lse.data_ptr(),
             dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), delta.data_ptr(), batch, q.shape[-2], k.shape[-2],
             total_q, total_k, q.shape[-1], *strides, cu_q.data_ptr() if cu_q is not None else None,
             cu_k.data_ptr() if cu_k is not None else None, seqlen_q, seqlen_k, int(bool(causal)),
             *win[:1]),
            win[1:] + (dsinks.data_ptr(),) if sinks is not None else ())  # `sinks, dsinks` after the stream

def flash_attention_varlen_backward(dout, q, k, v, out, lse, cu_seqlens_q, cu_seqlens_k=None,
                                    causal: bool = False, dq=None, dk=None, dv=None, stream=None,
                                    window: int = 0, sinks=None, dsinks=None):
    """Backward pass of :func:`flash_attention_varlen` (fa_attn_varlen_bwd_f16 /
    _bf16): the gradients of q, k and v from ``dout`` [T_q, Hq, D], the
    forward's inputs as it took them (views included), its ``out`` and its
    ``lse`` (return_lse=True: fp32 [Hq, T_q]).  dout follows q's stride rule and
    is never copied; anything that would need a copy raises.  GQA: dk and dv
    of a K/V head sum over its query heads, in fp32.  A row that saw no key
    gets dq = 0; a key no row sees gets dk = dv = 0; rows that belong to no
    sequence are neither read nor written (unspecified when the gradients are
    allocated here).  dq, dk, dv: contiguous tensors shaped like q, k, v, or
    None to allocate.  Returns (dq, dk, dv).  Three launches, no sync, one fp32
    [Hq, T_q] workspace allocated here, graph-capturable, and bit-reproducible:
    no atomics, no sum across workgroups.
    window, sinks: the forward's, whose out and lse these are
    (fa_attn_bwd_win_* / fa_attn_bwd_sink_*).  With a window the kernels walk
    the band, and a key no row sees gets dk = dv = 0.  With sinks (float32
    [Hq]) the return is (dq, dk, dv, dsinks): dsinks float32 [Hq], the
    gradient of the sinks, from a fourth launch in one fixed order (dsinks: a
    contiguous float32 [Hq] tensor to write, or None to allocate)."""
    window = _check_window(window, causal)  # before the tensors, as in the forward
    strides, grads, dsinks = _check_attn_bwd(dout, q, k, v, out, lse, 3, cu_seqlens_q, cu_seqlens_k, dq, dk,
                                             dv, sinks, dsinks)
    _attn_bwd_call(dout, q, k, v, out, lse, grads, strides, cu_seqlens_q.shape[0] - 1, q.shape[0],
                   k.shape[0], cu_seqlens_q, cu_seqlens_k, 0, 0, causal, stream, window, sinks, dsinks)
    return tuple(grads) if sinks is None else (*grads, dsinks)


def flash_attention_bshd_backward(dout, q, k, v, out, lse, causal: bool = False, dq=None, dk=None, dv=None,
                                  stream=None, window: int = 0, sinks=None, dsinks=None):
    """:func:`flash_attention_varlen_backward` for uniform lengths, the backward
    of :func:`flash_attention_bshd`: dout and q [B, Sq, Hq, D], k and v [B, Sk,
    Hkv, D], ``lse`` the [B, Hq, Sq] view that function returned (that view of
    a [Hq, B * Sq] buffer and no other layout).  Equals the packed function on
    cu_seqlens = arange(B + 1) * S bit for bit.  Returns (dq, dk, dv), or with
    sinks (dq, dk, dv, dsinks); window, sinks, dsinks: as for that function."""
    window = _check_window(window, causal)  # before the tensors, as in the forward
    strides, grads, dsinks = _check_attn_bwd(dout, q, k, v, out, lse, 4, None, None, dq, dk, dv, sinks,
                                             dsinks)
    b, sq = q.shape[0], q.shape[1]
    sk = k.shape[1]
    _attn_bwd_call(dout, q, k, v, out, lse, grads, strides, b, b * sq, b * sk, None, None, sq, sk, causal,
                   stream, window, sinks, dsinks)
    return tuple(grads) if sinks is None else (*grads, dsinks)


def flash_attn_varlen_func(q, k, v, cu_seqlens_q, cu_seqlens_k=None, causal: bool = False, window: int = 0,
                           sinks=None):
    """DIFFERENTIABLE attention over packed token-major q [T_q, Hq, D], k and v
    [T_k, Hkv, D], named as in flash-attn: :func:`flash_attention_varlen`
    forward, :func:`flash_attention_varlen_backward` under torch.autograd
    (fa_mi355x.torch_op, imported on first use).  Views as for the forward; a
    dout that fails the stride rule is made contiguous in backward (the one
    copy).  window, sinks: as for the forward; sinks may be a float32 [Hq]
    leaf that requires grad, whose .grad is the backward's dsinks.  No dropout."""
    from . import torch_op

    return torch_op.flash_attn_varlen_func(q, k, v, cu_seqlens_q, cu_seqlens_k, causal, window, sinks)


def flash_attn_func(q, k, v, causal: bool = False, window: int = 0, sinks=None):
    """:func:`flash_attn_varlen_func` for uniform lengths: q [B, Sq, Hq, D], k and
    v [B, Sk, Hkv, D] (:func:`flash_attention_bshd` and its backward)."""
    from . import torch_op

    return torch_op.flash_attn_func(q, k, v, causal, window, sinks)


def _append_varlen(k_new, v_new, k, v, block_table, names, cu_seqlens, kv_lens, k_scale, v_scale, stream):
    kv8, nseq = _check_packed(k_new, "k_new", v_new, "v_new", names[0], k, names[1], v, block_table,
                              cu_seqlens, "cu_seqlens", kv_lens, k_scale, v_scale, True)
    _append_call("fa_cache_append_varlen", kv8, k_new, v_new, k, v, nseq, k_new.shape[0], block_table,
                 kv_lens, cu_seqlens, stream, k_scale, v_scale)

def flash_attention_cache_append_varlen(k_new, v_new, k_cache, v_cache, cu_seqlens, kv_lens,
                                        k_scale=None, v_scale=None, stream=None) -> None:
    """:func:`flash_attention_cache_append` for a packed ragged batch
    (fa_cache_append_varlen_16, or fa_cache_append_varlen_kv8_* into an FP8
    cache).

    k_new, v_new: [T, Hkv, D], token-major, contiguous.  cu_seqlens: int32
    [B + 1], REQUIRED, read as :func:`flash_attention_prefill_varlen` reads
    cu_seqlens_q; B is the caches' batch.  kv_lens: int32 [B], REQUIRED, the
    lengths AFTER the append.  Token t of sequence b goes to cache row
    kv_lens[b] - n_b + t, written iff that row exists; the bytes, the FP8
    contract and "nothing else is touched" are the padded function's.  Read on
    the device: no sync, no workspace, graph-capturable.  Returns None.
    """
    _append_varlen(k_new, v_new, k_cache, v_cache, None, ("k_cache", "v_cache"), cu_seqlens, kv_lens,
                   k_scale, v_scale, stream)


def flash_attention_cache_append_varlen_paged(k_new, v_new, k_pages, v_pages, block_table, cu_seqlens,
                                              kv_lens, k_scale=None, v_scale=None, stream=None) -> None:
    """:func:`flash_attention_cache_append_varlen` into the page pools of
    :func:`flash_attention_cache_append_paged` (fa_cache_append_varlen_paged_16
    / _paged_kv8_*); B is the block table's row count.  Returns None."""
    if block_table is None:
        raise FlashAttentionError(FA_ERR_NULL_POINTER, "block_table is required")
    _append_varlen(k_new, v_new, k_pages, v_pages, block_table, ("k_pages", "v_pages"), cu_seqlens,
                   kv_lens, k_scale, v_scale, stream)


def _check_rope(x, xname, rank, q, q_out, cos, sin, where):
    """What the four rope_append wrappers check beyond the append's own checks.
    `where` false (before the append's checks, so before any device is looked
    at): cos and sin are contiguous float32 tensors of one shape [rope_len,
    R/2] with rope_len >= 1 and R a multiple of 16 in [16, D]; q (if given) and
    q_out (if given) are contiguous, of x's dtype and of x's shape but for the
    heads (x: k_new, [B,Hkv,Sn,D] with rank 4 or [T,Hkv,D] with rank 3).
    `where` true (after them): all four live on x's device and the tables are
    16-byte aligned."""
    import torch

    if where:
        for name, t in (("q", q), ("q_out", q_out), ("cos", cos), ("sin", sin)):
            if t is not None and (not t.is_cuda or t.device != x.device):
                raise FlashAttentionError(FA_ERR_NULL_POINTER, f"{name} must be a tensor on {x.device}")
        for name, t in (("cos", cos), ("sin", sin)):
            if t.data_ptr() % 16 != 0:
                raise FlashAttentionError(FA_ERR_BAD_SHAPE, f"{name} must be 16-byte aligned")
        return
    for name, t in (("cos", cos), ("sin", sin)):
        if not isinstance(t, torch.Tensor):
            raise FlashAttentionError(FA_ERR_NULL_POINTER,
                                      f"{name} is required: the float32 [rope_len, R/2] table")
        if t.dtype != torch.float32:
            raise FlashAttentionError(FA_ERR_BAD_SHAPE, f"{name} must be float32, got {t.dtype}")
        if t.dim() != 2 or not t.is_contiguous():
            raise FlashAttentionError(FA_ERR_BAD_SHAPE,
                                      f"{name} must be a contiguous [rope_len, R/2] tensor")
    if cos.shape != sin.shape:
        raise FlashAttentionError(
            FA_ERR_BAD_SHAPE, f"cos and sin must have one shape, got {list(cos.shape)} and {list(sin.shape)}")
    if cos.shape[0] < 1:
        raise FlashAttentionError(FA_ERR_BAD_SHAPE, "cos and sin hold no position (rope_len must be >= 1)")
    r = 2 * cos.shape[1]
    d = x.shape[-1] if x.dim() == rank else None
    if r < 16 or r % 16 != 0 or (d is not None and r > d):
        raise FlashAttentionError(
            FA_ERR_BAD_SHAPE,
            f"rotary_dim {r} (twice the tables' columns) is not a multiple of 16 in [16, head_dim]")
    if q is None:
        if q_out is not None:
            raise FlashAttentionError(FA_ERR_BAD_SHAPE, "q_out goes with q only")
        return
    layout = "[B,Hq,Sn,D]" if rank == 4 else "[T,Hq,D]"
    for name, t in (("q", q), ("q_out", q_out)):
        if t is None:
            continue
        if t.dtype != x.dtype:
            raise FlashAttentionError(FA_ERR_BAD_SHAPE, f"{name} must be {x.dtype} like {xname}, got {t.dtype}")
        if t.dim() != rank or not t.is_contiguous():
            raise FlashAttentionError(FA_ERR_BAD_SHAPE, f"{name} must be a contiguous {layout} tensor")
    if x.dim() == rank and (q.shape[:1] + q.shape[2:]) != (x.shape[:1] + x.shape[2:]):
        raise FlashAttentionError(
            FA_ERR_BAD_SHAPE,
            f"q must be {layout} with {xname}'s extents but for the heads, got {list(q.shape)} beside "
            f"{list(x.shape)}")
    if q_out is not None and q_out.shape != q.shape:
        raise FlashAttentionError(FA_ERR_BAD_SHAPE, "q_out must have q's shape")


def _rope_tail(q, q_out, cos, sin, interleaved):
    """The C entries' rotary arguments, after the append's."""
    return (q.data_ptr() if q is not None else None, q_out.data_ptr() if q is not None else None,
            q.shape[1] if q is not None else 0, cos.data_ptr(), sin.data_ptr(), cos.shape[0],
            2 * cos.shape[1], int(bool(interleaved)))


def _rope_append(q, k_new, v_new, k, v, block_table, names, kv_lens, cos, sin, new_lens, interleaved,
                 q_out, k_scale, v_scale, stream):
    _check_rope(k_new, "k_new", 4, q, q_out, cos, sin, False)
    kv8 = _check_append(k_new, v_new, names[0], k, names[1], v, block_table, kv_lens, new_lens,
                        k_scale, v_scale)
    if q is not None and q_out is None:
        import torch

        q_out = torch.empty_like(q)
    _check_rope(k_new, "k_new", 4, q, q_out, cos, sin, True)
    _append_call("fa_rope_append", kv8, k_new, v_new, k, v, k_new.shape[0], k_new.shape[2], block_table,
                 kv_lens, new_lens, stream, k_scale, v_scale, _rope_tail(q, q_out, cos, sin, interleaved))
    return q_out

def flash_attention_rope_append(q, k_new, v_new, k_cache, v_cache, kv_lens, cos, sin, new_lens=None,
                                interleaved: bool = False, q_out=None, k_scale=None, v_scale=None,
                                stream=None):
    """Rotary position embedding of Q and K fused with
    :func:`flash_attention_cache_append` (fa_rope_append_f16 / _bf16, or
    fa_rope_append_kv8_* into an FP8 cache): Q and K rotated, K and V appended,
    one launch.

    k_new, v_new, k_cache, v_cache, kv_lens, new_lens, the scales: as for
    :func:`flash_attention_cache_append`.  q: [B, Hq, Sn, D] of k_new's dtype,
    contiguous, or None (K/V only); Hq need not be a multiple of Hkv.  cos,
    sin: float32 [rope_len, R/2] device tensors, contiguous; R = rotary_dim, a
    multiple of 16 in [16, D].  Token t of element b has position pos =
    kv_lens[b] - n_b + t, the cache row the append writes (no positions tensor).
    interleaved False: NeoX / Hugging Face rotate_half pairs (x[i], x[i +
    R/2]); True: GPT-J pairs (x[2i], x[2i + 1]).  With c = cos[pos, i], s =
    sin[pos, i]: a' = a c - b s, b' = b c + a s, every product and sum one fp32
    operation, the result rounded once to the 16-bit type -- bit for bit what
    ``(a.float() * c - b.float() * s).to(dtype)`` gives on the CPU.  Elements
    at or past R are bit copies; V is appended unchanged.  The rotated 16-bit K
    row is what the append's contract stores, so the caches equal "rotate, then
    flash_attention_cache_append" byte for byte in all four forms.

    A K/V row is written iff the append's rule holds and pos < rope_len; a
    row of q_out iff 0 <= pos < rope_len (rows t >= n_b are not written:
    unspecified with q_out=None).  Returns q_out ([B, Hq, Sn, D]; allocated
    when None; ``q_out=q`` rotates in place), or None with q=None.  Everything
    is read on the device: no sync, no workspace, graph-capturable.
    """
    return _rope_append(q, k_new, v_new, k_cache, v_cache, None, ("k_cache", "v_cache"), kv_lens, cos,
                        sin, new_lens, interleaved, q_out, k_scale, v_scale, stream)


def flash_attention_rope_append_paged(q, k_new, v_new, k_pages, v_pages, block_table, kv_lens, cos, sin,
                                      new_lens=None, interleaved: bool = False, q_out=None,
                                      k_scale=None, v_scale=None, stream=None):
    """:func:`flash_attention_rope_append` into the page pools of
    :func:`flash_attention_cache_append_paged` (fa_rope_append_paged_* /
    fa_rope_append_paged_kv8_*).  An out-of-pool page id drops the K/V row, not
    the row of q_out."""
    if block_table is None:
        raise FlashAttentionError(FA_ERR_NULL_POINTER, "block_table is required")
    return _rope_append(q, k_new, v_new, k_pages, v_pages, block_table, ("k_pages", "v_pages"), kv_lens,
                        cos, sin, new_lens, interleaved, q_out, k_scale, v_scale, stream)


def _rope_append_varlen(q, k_new, v_new, k, v, block_table, names, cu_seqlens, kv_lens, cos, sin,
                        interleaved, q_out, k_scale, v_scale, stream):
    _check_rope(k_new, "k_new", 3, q, q_out, cos, sin, False)
    kv8, nseq = _check_packed(k_new, "k_new", v_new, "v_new", names[0], k, names[1], v, block_table,
                              cu_seqlens, "cu_seqlens", kv_lens, k_scale, v_scale, True)
    if q is not None and q_out is None:
        import torch

        q_out = torch.empty_like(q)
    _check_rope(k_new, "k_new", 3, q, q_out, cos, sin, True)
    _append_call("fa_rope_append_varlen", kv8, k_new, v_new, k, v, nseq, k_new.shape[0], block_table,
                 kv_lens, cu_seqlens, stream, k_scale, v_scale, _rope_tail(q, q_out, cos, sin, interleaved))
    return q_out

def flash_attention_rope_append_varlen(q, k_new, v_new, k_cache, v_cache, cu_seqlens, kv_lens, cos, sin,
                                       interleaved: bool = False, q_out=None, k_scale=None,
                                       v_scale=None, stream=None):
    """:func:`flash_attention_rope_append` for a packed ragged batch
    (fa_rope_append_varlen_*): q [T, Hq, D] (or None), k_new and v_new [T, Hkv,
    D], token-major; cu_seqlens and kv_lens as for
    :func:`flash_attention_cache_append_varlen`.  Token t of sequence b (packed
    row s_b + t) has position kv_lens[b] - n_b + t.  The caches and the rows of
    q_out equal the padded function's bit for bit; rows of q_out that belong to
    no sequence are not written.  Returns q_out [T, Hq, D], or None."""
    return _rope_append_varlen(q, k_new, v_new, k_cache, v_cache, None, ("k_cache", "v_cache"),
                               cu_seqlens, kv_lens, cos, sin, interleaved, q_out, k_scale, v_scale, stream)


def flash_attention_rope_append_varlen_paged(q, k_new, v_new, k_pages, v_pages, block_table, cu_seqlens,
                                             kv_lens, cos, sin, interleaved: bool = False, q_out=None,
                                             k_scale=None, v_scale=None, stream=None):
    """:func:`flash_attention_rope_append_varlen` into the page pools of
    :func:`flash_attention_cache_append_paged` (fa_rope_append_varlen_paged_*);
    B is the block table's row count."""
    if block_table is None:
        raise FlashAttentionError(FA_ERR_NULL_POINTER, "block_table is required")
    return _rope_append_varlen(q, k_new, v_new, k_pages, v_pages, block_table, ("k_pages", "v_pages"),
                               cu_seqlens, kv_lens, cos, sin, interleaved, q_out, k_scale, v_scale, stream)


def splitkv_buffers(batch: int, heads: int, seq_len: int, num_splits: int, device="cuda"):
    """Allocate the reference-layout split-K buffers (O partials, (m,l))."""
    import torch

    rows = batch * heads * seq_len
    part_o = torch.empty(num_splits * rows * HEAD_DIM, dtype=torch.float32, device=device)
    part_ml = torch.empty(num_splits * rows * 2, dtype=torch.float32, device=device)
    return part_o, part_ml


def flash_attention_fwd_splitkv(q, k, v, causal: bool = False, num_splits: int = 0, out=None,
                                part_o=None, part_ml=None, stream=None):
    """Split-KV forward + log-sum-exp merge (ref split-K path, :169-180/:559-598)."""
    import torch

    # the split-KV entry is fp16-only (fa_fwd_f16_splitkv takes untyped
    # pointers, as the reference's half* split-K path does, :606-611): a bf16
    # tensor would be read as fp16 bits, so reject it before anything else
    if q.dtype != torch.float16:
        raise FlashAttentionError(FA_ERR_BAD_SHAPE,
                                  f"split-KV takes float16 tensors only, got {q.dtype}")
    if out is None:
        out = torch.empty_like(q)
    _check_qkvo(q, k, v, out)
    b, h, s, d = q.shape
    lib = load_library()
    if num_splits <= 0:
        num_splits = lib.fa_splitkv_num_splits(b, h, s, int(bool(causal)))
    if part_o is None or part_ml is None:
        part_o, part_ml = splitkv_buffers(b, h, s, num_splits, device=q.device)
    need_o = lib.fa_splitkv_o_bytes(b, h, s, d, num_splits)
    need_ml = lib.fa_splitkv_ml_bytes(b, h, s, d, num_splits)
    if part_o.numel() * 4 < need_o or part_ml.numel() * 4 < need_ml:
        raise FlashAttentionError(FA_ERR_WORKSPACE, "split-KV buffers too small")
    for name, t in (("part_o", part_o), ("part_ml", part_ml)):
        if t.device != q.device or t.dtype != torch.float32 or not t.is_contiguous():
            raise FlashAttentionError(FA_ERR_WORKSPACE,
                                      f"{name} must be contiguous float32 on {q.device}")
    with torch.cuda.device(q.device):
        st = ctypes.c_void_p(_raw_stream(stream, q.device.index))
        _check(lib.fa_fwd_f16_splitkv(
            ctypes.c_void_p(q.data_ptr()), ctypes.c_void_p(k.data_ptr()),
            ctypes.c_void_p(v.data_ptr()), ctypes.c_void_p(out.data_ptr()), b, h, s, d,
            int(bool(causal)), int(num_splits), ctypes.c_void_p(part_o.data_ptr()),
            ctypes.c_void_p(part_ml.data_ptr()), st))
    return out


def flash_attention_v9_dispatch(Q, K, V, Output, splitk_buf_O, splitk_buf_ml, batch_size: int,
                                num_heads: int, seq_len: int, head_dim: int, causal: bool,
                                stream=0):
    """Mirror of the reference host launch signature (flash_attention.cu:606-611).

    Q/K/V/Output are device tensors (or raw device pointers as ints) holding
    BHSD fp16 data on the current device.  splitk_buf_O/splitk_buf_ml are
    accepted and ignored, as the reference's dispatcher ignores them (it only
    launches split_k = 1; split-KV is :func:`flash_attention_fwd_splitkv`).
    Raises FlashAttentionError where the reference would exit(EXIT_FAILURE).
    """
    del splitk_buf_O, splitk_buf_ml

    # the reference's boundary is typed half* (:606-611): tensors must be
    # float16 (raw pointers cannot be checked and are taken as fp16 BHSD)
    for name, x in (("Q", Q), ("K", K), ("V", V), ("Output", Output)):
        if not isinstance(x, int):
            import torch

            if x.dtype != torch.float16:
                raise FlashAttentionError(FA_ERR_BAD_SHAPE, f"{name} must be float16, got {x.dtype}")

    def ptr(x):
        return x if isinstance(x, int) else x.data_ptr()

    lib = load_library()
    st = ctypes.c_void_p(_raw_stream(stream, None) if stream not in (0, None) else None)  # (0, None: the null stream)
    q, k, v, o = (ctypes.c_void_p(ptr(x)) for x in (Q, K, V, Output))
    _check(lib.fa_fwd_f16(q, k, v, o, batch_size, num_heads, seq_len, head_dim,
                          int(bool(causal)), st))


def attention_flops(batch: int, heads: int, seq_len: int, head_dim: int, causal: bool) -> float:
    """Reference FLOP convention: 4*B*H*S^2*D, halved when causal (:938-939)."""
    f = 4.0 * batch * heads * seq_len * seq_len * head_dim
    return f / 2 if causal else f


def kernel_symbol(config_name: str) -> str:
    """Substring of the kernel symbol rocprofv3 reports for a tile config."""
    if "_asm_persistent" in config_name:
        return "fa_fwd_f16_w4_kernel"
    if "persistent" in config_name:
        return "fa_fwd_f16_persistent_kernel"
    if "kvpair" in config_name or "kvquad" in config_name:
        return "fa_fwd_f16_kvpair_kernel"
    if "splitkv" in config_name:
        return "fa_fwd_f16_splitkv_kernel"
    return "fa_fwd_f16_kernel"
