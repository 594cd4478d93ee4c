"""C-ABI checks that several CPU test files run: the export check, the
compile-time resource usage of a csrc unit, and the argument tables of the two
16-bit decode entries (which the FP8 entries must answer alike)."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "flash-attention-cuda_amd")
HIPCC = "/opt/rocm/bin/hipcc"
# the Makefile's HIPFLAGS but for -Wall: what decides a kernel's registers, scratch and LDS
HIPFLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fno-honor-nans",
            "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(PKG, "csrc")]
MAX_SPLITS = 64  # the plan's upper cap (csrc/fa_decode_host.hpp kDecodeMaxSplits)
INT_MAX = 2 ** 31 - 1


def fa():
    import fa_mi355x

    return fa_mi355x


def header_text(header):
    """A public header's text without its comments."""
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return re.sub(r"//.*", "", text)


def exported_symbols():
    """The dynamic symbols the built library defines."""
    out = subprocess.run(["nm", "-D", "--defined-only", fa().library_path()], capture_output=True,
                         text=True, check=True).stdout
    return {line.split()[-1] for line in out.splitlines() if line.strip()}


def assert_exported(symbols):
    """Each symbol is defined by the library, listed in EXPORTED_SYMBOLS and
    declared as a function in include/fa_mi355x.h."""
    syms = exported_symbols()
    header = open(os.path.join(ROOT, "include", "fa_mi355x.h")).read()
    for s in symbols:
        assert s in syms, s
        assert s in fa().EXPORTED_SYMBOLS, s
        assert re.search(r"\b%s\s*\(" % s, header), s


def kernel_resource_usage(units, timeout=600):
    """hipcc's kernel-resource-usage remarks of the named csrc units, compiled
    for gfx950 side by side: per unit a list of (kernel name, scratch bytes per
    lane, LDS bytes per block), in the compiler's order.  `timeout` is per unit."""
    procs = [subprocess.Popen([HIPCC, *HIPFLAGS, "-c", os.path.join(PKG, "csrc", unit), "-o", os.devnull,
                               "-Rpass-analysis=kernel-resource-usage"],
                              stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for unit in units]
    out = []
    try:
        for unit, proc in zip(units, procs):
            _, err = proc.communicate(timeout=timeout)
            assert proc.returncode == 0, (unit, err[-2000:])
            names = re.findall(r"Function Name: (\S+)", err)
            scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", err)]
            lds = [int(x) for x in re.findall(r"LDS Size \[bytes/block\]: (\d+)", err)]
            assert len(names) == len(scratch) == len(lds), (unit, len(names), len(scratch), len(lds))
            out.append(list(zip(names, scratch, lds)))
    finally:
        for proc in procs:
            if proc.poll() is None:
                proc.kill()
    return out


def _decode_call(fn, q, k, v, o, b, hq, hkv, sq, cap, d, lens=None, causal=1, ns=0, ws=None, wsb=0):
    return fn(q, k, v, o, None, b, hq, hkv, sq, cap, d, lens, causal, ns, ws, wsb, None)


def decode_argument_checks(fa, lib):
    """The contiguous decode entries' statuses, all returned before any launch
    (fake pointers).  fa: the FA_* constants; lib: fa_decode_f16 / _bf16 and
    fa_decode_ws_bytes (the loaded library, or a shim that binds other entries
    to those names)."""
    _call = _decode_call
    p = ctypes.c_void_p(0x1000)
    for fn in (lib.fa_decode_f16, lib.fa_decode_bf16):
        for bad in range(4):  # each of q, k, v, o NULL in turn
            ptrs = [None if i == bad else p for i in range(4)]
            assert _call(fn, *ptrs, 1, 8, 2, 1, 1024, 128) == fa.FA_ERR_NULL_POINTER
        for d in (0, 32, 96, 256):
            assert _call(fn, p, p, p, p, 1, 8, 2, 1, 1024, d) == fa.FA_ERR_UNSUPPORTED_HEAD_DIM
        for hq, hkv in ((8, 3), (7, 2), (4, 8)):
            assert _call(fn, p, p, p, p, 1, hq, hkv, 1, 1024, 128) == fa.FA_ERR_BAD_SHAPE
        for sq in (0, 17, -1):
            assert _call(fn, p, p, p, p, 1, 8, 2, sq, 1024, 128) == fa.FA_ERR_BAD_SHAPE
        assert _call(fn, p, p, p, p, -1, 8, 2, 1, 1024, 128) == fa.FA_ERR_BAD_SHAPE
        assert _call(fn, p, p, p, p, 1, -8, 2, 1, 1024, 128) == fa.FA_ERR_BAD_SHAPE
        assert _call(fn, p, p, p, p, 1, 8, -2, 1, 1024, 128) == fa.FA_ERR_BAD_SHAPE
        assert _call(fn, p, p, p, p, 1, 8, 2, 1, -5, 128) == fa.FA_ERR_BAD_SHAPE
        # cap * 2 * head_dim past INT_MAX
        assert _call(fn, p, p, p, p, 1, 8, 2, 1, 8388608, 128) == fa.FA_ERR_BAD_SHAPE
        assert _call(fn, p, p, p, p, 1, 8, 2, 1, 16777216, 64) == fa.FA_ERR_BAD_SHAPE
        # no kv_lens, causal, fewer cache rows than query tokens
        assert _call(fn, p, p, p, p, 1, 8, 2, 4, 3, 128, None, 1) == fa.FA_ERR_BAD_SHAPE
        # splitting needs a workspace: present, long enough, 16-byte aligned
        need = lib.fa_decode_ws_bytes(1, 8, 2, 1, 4096, 128, 4)
        assert need > 65536
        assert _call(fn, p, p, p, p, 1, 8, 2, 1, 4096, 128, ns=4) == fa.FA_ERR_WORKSPACE
        assert _call(fn, p, p, p, p, 1, 8, 2, 1, 4096, 128, ns=4, ws=p, wsb=need - 1) == \
            fa.FA_ERR_WORKSPACE
        assert _call(fn, p, p, p, p, 1, 8, 2, 1, 4096, 128, ns=4, ws=ctypes.c_void_p(0x1008),
                     wsb=need) == fa.FA_ERR_WORKSPACE
        # more pieces than the cap
        assert _call(fn, p, p, p, p, 1, 8, 2, 1, 4096, 128, ns=MAX_SPLITS + 1, ws=p,
                     wsb=1 << 40) == fa.FA_ERR_BAD_CONFIG
        # empty problems: nothing to do, nothing launched, no pointer looked at
        assert _call(fn, None, None, None, None, 0, 8, 2, 1, 1024, 128) == fa.FA_OK
        assert _call(fn, None, None, None, None, 1, 0, 0, 1, 1024, 128) == fa.FA_OK


def _paged_call(fn, q, k, v, o, b, hq, hkv, sq, d, npages, psz, table, mpp, lens=None, causal=1, ns=0,
                ws=None, wsb=0):
    return fn(q, k, v, o, None, b, hq, hkv, sq, d, npages, psz, table, mpp, lens, causal, ns, ws, wsb,
              None)


def decode_paged_argument_checks(fa, lib):
    """The paged decode entries' statuses, all returned before any launch (fake
    pointers).  fa: the FA_* constants; lib: fa_decode_paged_f16 / _bf16,
    fa_decode_ws_bytes and fa_decode_num_splits (the loaded library, or a shim
    that binds other entries to those names)."""
    _call = _paged_call
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


# The attention entries the three host bodies serve: family x variant x cache
# form x element type (the fa_attn_varlen_* entries read no cache: one form).
FORMS = ("", "_paged", "_kv8", "_paged_kv8")
VARIANTS = ("", "_win", "_sink")
ATTENTION_ENTRIES = [(fam, var, form, ty)
                     for fam in ("fa_decode", "fa_prefill", "fa_prefill_varlen", "fa_attn_varlen")
                     for var in VARIANTS for form in (FORMS if fam != "fa_attn_varlen" else ("",))
                     for ty in ("_f16", "_bf16")]


def entry_symbol(entry):
    fam, var, form, ty = entry
    return fam + var + form + ty


def _entry_call(lib, entry, q=None, k=None, v=None, o=None, table=None, qlens=None, b=1, hq=2, hkv=1,
                sq=1, cap=128, d=64, psz=64, causal=1, window=0):
    """One attention entry on the shared arguments, each argument group where
    its list has it: the paged forms take `cap` as two pages of `psz` keys from
    a pool of two, the token-major entries as uniform lengths (totals = b * sq
    and b * cap, no cu_seqlens)."""
    fam, var, form, _ = entry
    fn = getattr(lib, entry_symbol(entry))
    win = {"": [], "_win": [window], "_sink": [window, None]}[var]
    scales = [None, None] if "kv8" in form else []
    if fam == "fa_attn_varlen":
        return fn(q, k, v, o, None, b, hq, hkv, b * sq, b * cap, d, 0, 0, 0, None, None, sq, cap, causal,
                  *win[:1], None, *win[1:])
    cache = [d, 2, psz, table, 2] if "paged" in form else [cap, d]
    if fam == "fa_decode":
        return fn(q, k, v, o, None, b, hq, hkv, sq, *cache, None, causal, *win, 0, None, 0, None, *scales)
    return fn(q, k, v, o, None, b, hq, hkv, sq, *cache, None, qlens, causal, *win, None, *scales)


def entry_status_checks(fa, lib, entry):
    """The argument statuses every attention entry answers alike, whichever
    argument groups its list carries; all are returned before any HIP call
    (fake pointers).  B=1, Hq=2, Hkv=1, cap=128, D=64; Sq=1 for decode, else 130."""
    fam, var, form, _ = entry
    p = ctypes.c_void_p(0x1000)
    sq = 1 if fam == "fa_decode" else 130
    ptrs = dict(q=p, k=p, v=p, o=p, table=p, qlens=p)

    def call(**kw):
        return _entry_call(lib, entry, **{"sq": sq, **ptrs, **kw})

    # negative extents
    assert call(b=-1) == fa.FA_ERR_BAD_SHAPE
    assert call(hq=-2) == fa.FA_ERR_BAD_SHAPE
    assert call(hkv=-1) == fa.FA_ERR_BAD_SHAPE
    assert call(d=96) == fa.FA_ERR_UNSUPPORTED_HEAD_DIM
    # an empty batch: nothing to do, no pointer looked at
    assert _entry_call(lib, entry, b=0, sq=sq) == fa.FA_OK
    if var:
        assert call(window=-1) == fa.FA_ERR_BAD_SHAPE
        assert call(window=4, causal=0) == fa.FA_ERR_BAD_SHAPE
    if "paged" in form:
        assert call(psz=32) == fa.FA_ERR_BAD_SHAPE
    # a valid shape: q is looked at after every shape check
    assert call(q=None) == fa.FA_ERR_NULL_POINTER
