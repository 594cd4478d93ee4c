"""GPU tests of every decode kernel instantiation, split and unsplit, against a
reference that is not this kernel (fa_decode_* and fa_decode_paged_*:
T in {fp16, bf16} x HDIM in {64, 128} x NB in {1, 2, 4} x {contiguous, paged}).

The table below is the plain 16-bit quarter of the decode instantiations: the
FP8 forms, the `_win` and `_sink` twins and the tree entries multiply it to 192
kernels.  tests/instantiation_matrix.py lists all of them with the prefill and
no-cache families (300 cells) and tests/test_instantiation_matrix_gpu.py holds
each to a closed form.

Helpers, references and gates are those of tests/decode_refs.py; no new
tolerance:
  * fp16 O: the CPU oracle, 1e-3.
  * bf16 O: fp32 torch on the same bf16 inputs, 5e-3.
  * LSE: float64 reference, 2^-10 * max|scaled score| + 1e-5.
  * a row that sees no key: O exactly zero, LSE exactly -inf.

Coverage (NB = 16-row blocks per workgroup: 1 for G*Sq <= 16, 2 for <= 32,
else 4; "matrix" is test_variant_split_matrix[dtype-d-G-Sq], which runs the
contiguous entry with num_splits 1 / 2, 3, 7 (causal and not) and the paged
entry with num_splits 1 / 3 (causal)):

  dtype  d    NB  entry       unsplit                 split
  fp16   128  1   contiguous  matrix[fp16-128-5-1]    matrix[fp16-128-5-1]
  fp16   128  1   paged       matrix[fp16-128-5-1]    matrix[fp16-128-5-1]
  fp16   128  2   contiguous  matrix[fp16-128-7-3]    matrix[fp16-128-7-3]
  fp16   128  2   paged       matrix[fp16-128-7-3]    matrix[fp16-128-7-3]
  fp16   128  4   contiguous  matrix[fp16-128-4-16]   matrix[fp16-128-4-16]
  fp16   128  4   paged       matrix[fp16-128-4-16]   matrix[fp16-128-4-16]
  fp16   64   1   contiguous  matrix[fp16-64-5-1]     matrix[fp16-64-5-1]
  fp16   64   1   paged       matrix[fp16-64-5-1]     matrix[fp16-64-5-1]
  fp16   64   2   contiguous  matrix[fp16-64-7-3]     matrix[fp16-64-7-3]
  fp16   64   2   paged       matrix[fp16-64-7-3]     matrix[fp16-64-7-3]
  fp16   64   4   contiguous  matrix[fp16-64-4-16]    matrix[fp16-64-4-16]
  fp16   64   4   paged       matrix[fp16-64-4-16]    matrix[fp16-64-4-16]
  bf16   128  1   contiguous  matrix[bf16-128-5-1]    matrix[bf16-128-5-1]
  bf16   128  1   paged       matrix[bf16-128-5-1]    matrix[bf16-128-5-1]
  bf16   128  2   contiguous  matrix[bf16-128-7-3]    matrix[bf16-128-7-3]
  bf16   128  2   paged       matrix[bf16-128-7-3]    matrix[bf16-128-7-3]
  bf16   128  4   contiguous  matrix[bf16-128-4-16]   matrix[bf16-128-4-16]
  bf16   128  4   paged       matrix[bf16-128-4-16]   matrix[bf16-128-4-16]
  bf16   64   1   contiguous  matrix[bf16-64-5-1]     matrix[bf16-64-5-1]
  bf16   64   1   paged       matrix[bf16-64-5-1]     matrix[bf16-64-5-1]
  bf16   64   2   contiguous  matrix[bf16-64-7-3]     matrix[bf16-64-7-3]
  bf16   64   2   paged       matrix[bf16-64-7-3]     matrix[bf16-64-7-3]
  bf16   64   4   contiguous  matrix[bf16-64-4-16]    matrix[bf16-64-4-16]
  bf16   64   4   paged       matrix[bf16-64-4-16]    matrix[bf16-64-4-16]

matrix[*-16-5] runs every NB = 4 instantiation once more with a second row
group (80 rows: 64 + 16).  The remaining tests: rows that some or all pieces
cannot see (test_rows_unseen_by_pieces), the kv_lens clamp of both entries
(test_kv_lens_clamp_*), stores outside O, LSE and the promised workspace
(test_no_write_outside_*) and a non-default stream (test_non_default_stream).
"""
import numpy as np
import pytest
import torch

import decode_refs as dr
import fa_mi355x

pytestmark = pytest.mark.gpu

DEV = "cuda"
K_PAD, V_PAD = 0x7fff, -1   # int16 bit patterns (0x7fff, 0xffff): NaN in fp16 and in bf16
O_SENTINEL = 0x7fff         # 16-bit guard pattern around O
LSE_SENTINEL = 0x7fa5a5a5   # 32-bit guard pattern around LSE (a NaN: never a result)
GUARD = 64                  # guard rows of O / guard floats of LSE on either side
WS_GUARD = 4096             # bytes of 0xA5 behind the promised workspace

decode = fa_mi355x.flash_attention_decode
decode_paged = fa_mi355x.flash_attention_decode_paged


def _case(b, hq, hkv, sq, cap, d, lens, dtype):
    """The oracle generator's inputs as (numpy fp16 bits, device tensors of
    `dtype`); the device caches' rows past each length hold NaN bit patterns."""
    q, k, v = dr.inputs(b, hq, hkv, sq, cap, d)
    tq, tk, tv = (dr.dev(a).to(dtype) for a in (q, k, v))
    for i, n in enumerate(lens):
        tk[i, :, int(n):].view(torch.int16).fill_(K_PAD)
        tv[i, :, int(n):].view(torch.int16).fill_(V_PAD)
    return (q, k, v), (tq, tk, tv)


# ---- 1. every variant, split and unsplit --------------------------------------------

MATRIX_LENS = (70, 300, 640)


@pytest.mark.parametrize("g,sq", [(5, 1), (7, 3), (4, 16), (16, 5)])
@pytest.mark.parametrize("d", [128, 64])
@pytest.mark.parametrize("dtype", dr.DTYPES)
def test_variant_split_matrix(dtype, d, g, sq):
    """5 / 21 / 64 / 80 rows per K/V head (NB = 1 / 2 / 4 / 4 with a second row
    group).  70 keys are 2 tiles (7 pieces: five are empty; Sq = 16 causal: rows
    t < 10 see nothing of tile 1), 300 are 5 (3 pieces: 1 / 2 / 2 tiles), 640 are
    10 (2 pieces: wave 0 runs a second round)."""
    b, hkv, cap = 3, 2, 640
    lens = np.array(MATRIX_LENS)
    host, dev = _case(b, hkv * g, hkv, sq, cap, d, lens, dtype)
    tl = dr.lens(lens)
    tag = f"{dr.name(dtype)} d={d} NB={dr.nb(g, sq)} G={g} Sq={sq}"
    refs = {}
    for causal in (True, False):
        refs[causal] = dr.refs(host, dev, lens, causal, dtype)
        for ns in (1, 2, 3, 7):
            out, lse = decode(*dev, tl, causal=causal, return_lse=True, num_splits=ns)
            dr.check(out, lse, refs[causal], dtype, f"contig {tag} causal={causal} ns={ns}")
            if ns > 1:
                assert dr.ws_counters_zero(), (tag, causal, ns)
    kp, vp, table = dr.paginate(dev[1], dev[2], 128, lens)
    for ns in (1, 3):
        out, lse = decode_paged(dev[0], kp, vp, table, tl, causal=True, return_lse=True,
                                num_splits=ns)
        dr.check(out, lse, refs[True], dtype, f"paged {tag} causal=True ns={ns}")
        if ns > 1:
            assert dr.ws_counters_zero(), (tag, "paged", ns)


# ---- 2. rows that no piece, or only some pieces, can see ----------------------------

UNSEEN = [
    (16, 70),   # tile 1 is masked for rows t < 10, live for the rest: -inf beside finite LSEs
    (16, 16),   # row 0 sees one key
    (16, 17),   # one key more than Sq
    (5, 3),     # two rows see nothing in any piece; with 2 pieces piece 0 has no tile
    (16, 129),  # three tiles; the last holds one key that only the last row sees
]


@pytest.mark.parametrize("sq,n", UNSEEN)
@pytest.mark.parametrize("dtype", dr.DTYPES)
def test_rows_unseen_by_pieces(dtype, sq, n):
    lens = np.array([n])
    host, dev = _case(1, 2, 1, sq, 192, 128, lens, dtype)
    refs = dr.refs(host, dev, lens, True, dtype)
    if (sq, n) == (5, 3):
        assert np.isneginf(refs[1][:, :, :2]).all() and np.isfinite(refs[1][:, :, 2:]).all()
    for ns in (2, 3):
        out, lse = decode(*dev, dr.lens(lens), causal=True, return_lse=True, num_splits=ns)
        dr.check(out, lse, refs, dtype, f"unseen {dr.name(dtype)} Sq={sq} len={n} ns={ns}")
        assert dr.ws_counters_zero(), (sq, n, ns)


# ---- 3. the kv_lens clamp -----------------------------------------------------------

@pytest.mark.parametrize("ns", [1, 2])
def test_kv_lens_clamp_contiguous(ns):
    """Lengths below 0 and above the capacity act as 0 and the capacity.  The
    caches are the middle elements of a larger allocation whose outer elements
    are NaN: an unclamped length reads the next head or NaN, nothing else."""
    b, hq, hkv, sq, cap, d = 4, 8, 2, 2, 192, 128
    q, k, v = dr.inputs(b, hq, hkv, sq, cap, d)
    tq = dr.dev(q)
    bigk = dr.nan_fill(torch.empty((b + 2, hkv, cap, d), dtype=torch.float16, device=DEV))
    bigv = dr.nan_fill(torch.empty_like(bigk))
    tk, tv = bigk[1:1 + b], bigv[1:1 + b]
    tk.copy_(dr.dev(k))
    tv.copy_(dr.dev(v))
    assert tk.is_contiguous() and tv.is_contiguous()
    clamped = np.array([0, 0, 192, 192])
    want = decode(tq, tk, tv, dr.lens(clamped), causal=True, return_lse=True, num_splits=ns)
    got = decode(tq, tk, tv, dr.lens([-1, -64, 193, 256]), causal=True, return_lse=True,
                 num_splits=ns)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    refs = (dr.oracle_decode(q, k, v, clamped, True),) + dr.lse_ref(q, k, v, clamped, True)
    dr.check(want[0], want[1], refs, torch.float16, f"clamp contig ns={ns}")


@pytest.mark.parametrize("ns", [1, 2])
def test_kv_lens_clamp_paged(ns):
    """The same over pages of 64 keys, three per sequence.  The block table is
    the middle rows of a larger one whose outer rows name NaN pages: an
    unclamped length reads the next row's first entry."""
    b, hq, hkv, sq, cap, d = 4, 8, 2, 2, 192, 128
    q, k, v = dr.inputs(b, hq, hkv, sq, cap, d)
    tq, tk, tv = dr.dev(q), dr.dev(k), dr.dev(v)
    clamped = np.array([0, 192, 192, 192])
    kp, vp, table = dr.paginate(tk, tv, 64, clamped, seed=21)
    free = sorted(set(range(kp.shape[0])) - set(table[1:].flatten().tolist()))
    assert len(free) >= 3 and bool(torch.isnan(kp[free[-3:]]).all())  # pages no sequence uses
    big = torch.tensor([free[-3:]] * (b + 2), dtype=torch.int32, device=DEV)
    big[1:1 + b] = table
    tab = big[1:1 + b]
    assert tab.is_contiguous()
    want = decode_paged(tq, kp, vp, tab, dr.lens(clamped), causal=True, return_lse=True,
                        num_splits=ns)
    got = decode_paged(tq, kp, vp, tab, dr.lens([-1, 193, 256, 192]), causal=True, return_lse=True,
                       num_splits=ns)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    refs = (dr.oracle_decode(q, k, v, clamped, True),) + dr.lse_ref(q, k, v, clamped, True)
    dr.check(want[0], want[1], refs, torch.float16, f"clamp paged ns={ns}")


# ---- 4. nothing is written outside O, LSE or the promised workspace -----------------

def _guarded_o(b, hq, sq, d, dtype):
    buf = torch.empty((GUARD + b * hq * sq + GUARD, d), dtype=dtype, device=DEV)
    buf.view(torch.int16).fill_(O_SENTINEL)
    return buf, buf[GUARD:GUARD + b * hq * sq].view(b, hq, sq, d)


def _guarded_lse(b, hq, sq):
    buf = torch.empty(GUARD + b * hq * sq + GUARD, dtype=torch.float32, device=DEV)
    buf.view(torch.int32).fill_(LSE_SENTINEL)
    return buf, buf[GUARD:GUARD + b * hq * sq].view(b, hq, sq)


def _guarded_ws(need):
    buf = torch.zeros(need + WS_GUARD, dtype=torch.uint8, device=DEV)
    buf[need:] = 0xA5
    return buf


def _guards_intact(obuf, lbuf, wsbuf, need):
    """Every sentinel around O (and LSE and the workspace, where given) is in
    place and the workspace's counter region is zero."""
    torch.cuda.synchronize()
    ob = obuf.view(torch.int16)
    ok = bool((ob[:GUARD] == O_SENTINEL).all()) and bool((ob[-GUARD:] == O_SENTINEL).all())
    if lbuf is not None:
        lb = lbuf.view(torch.int32)
        ok = ok and bool((lb[:GUARD] == LSE_SENTINEL).all()) and bool((lb[-GUARD:] == LSE_SENTINEL).all())
    if wsbuf is not None:
        ok = (ok and bool((wsbuf[need:] == 0xA5).all())
              and int(torch.count_nonzero(wsbuf[:min(need, 65536)]).item()) == 0)
    return ok


@pytest.mark.parametrize("g,sq", [(5, 1), (7, 3), (16, 5)])
@pytest.mark.parametrize("dtype,d", [pytest.param(torch.float16, 128, id="fp16-128"),
                                     pytest.param(torch.bfloat16, 64, id="bf16-64")])
def test_no_write_outside_outputs_or_workspace(dtype, d, g, sq):
    """The C entries with O, LSE and the workspace in the middle of guarded
    buffers: padded rows of a row group and the split's slabs stay inside."""
    b, hkv, cap, n = 2, 2, 320, 300
    hq = hkv * g
    lens = np.array([n] * b)
    _, (tq, tk, tv) = _case(b, hq, hkv, sq, cap, d, lens, dtype)
    tl = dr.lens(lens)
    kp, vp, table = dr.paginate(tk, tv, 64, lens, seed=31)
    lib = fa_mi355x.load_library()
    bf16 = dtype is torch.bfloat16
    st = torch.cuda.current_stream().cuda_stream
    for ns in (1, 3):
        need = lib.fa_decode_ws_bytes(b, hq, hkv, sq, cap, d, ns)
        assert (need == 0) == (ns == 1)
        for entry in ("contig", "paged"):
            what = f"guards {entry} {dr.name(dtype)} d={d} G={g} Sq={sq} ns={ns}"
            if entry == "contig":
                want = decode(tq, tk, tv, tl, causal=True, return_lse=True, num_splits=ns)
            else:
                want = decode_paged(tq, kp, vp, table, tl, causal=True, return_lse=True,
                                    num_splits=ns)
            obuf, o = _guarded_o(b, hq, sq, d, dtype)
            lbuf, lse = _guarded_lse(b, hq, sq)
            ws = _guarded_ws(need)
            if entry == "contig":
                rc = (lib.fa_decode_bf16 if bf16 else lib.fa_decode_f16)(
                    tq.data_ptr(), tk.data_ptr(), tv.data_ptr(), o.data_ptr(), lse.data_ptr(),
                    b, hq, hkv, sq, cap, d, tl.data_ptr(), 1, ns, ws.data_ptr(), need, st)
            else:
                rc = (lib.fa_decode_paged_bf16 if bf16 else lib.fa_decode_paged_f16)(
                    tq.data_ptr(), kp.data_ptr(), vp.data_ptr(), o.data_ptr(), lse.data_ptr(),
                    b, hq, hkv, sq, d, kp.shape[0], kp.shape[2], table.data_ptr(), table.shape[1],
                    tl.data_ptr(), 1, ns, ws.data_ptr(), need, st)
            assert rc == fa_mi355x.FA_OK, (what, rc)
            assert _guards_intact(obuf, lbuf, ws, need), what
            assert torch.equal(o, want[0]) and torch.equal(lse, want[1]), what
        # the Python entries write into the caller's `out` and return it
        for entry in ("contig", "paged"):
            obuf, o = _guarded_o(b, hq, sq, d, dtype)
            if entry == "contig":
                got = decode(tq, tk, tv, tl, causal=True, out=o, num_splits=ns)
                want = decode(tq, tk, tv, tl, causal=True, num_splits=ns)
            else:
                got = decode_paged(tq, kp, vp, table, tl, causal=True, out=o, num_splits=ns)
                want = decode_paged(tq, kp, vp, table, tl, causal=True, num_splits=ns)
            assert got is o, (entry, ns)
            assert _guards_intact(obuf, None, None, 0), (entry, g, sq, ns)
            assert torch.equal(o, want), (entry, ns)


# ---- 5. a stream that is not the current one ----------------------------------------

def test_non_default_stream():
    """stream= another stream: the default stream's bits, that stream's own
    workspace, its counters back to zero."""
    b, hkv, g, sq, cap, d = 3, 2, 7, 3, 640, 128
    lens = np.array(MATRIX_LENS)
    _, (tq, tk, tv) = _case(b, hkv * g, hkv, sq, cap, d, lens, torch.float16)
    tl = dr.lens(lens)
    want = decode(tq, tk, tv, tl, causal=True, return_lse=True, num_splits=3)
    s = torch.cuda.Stream()
    assert s.cuda_stream != torch.cuda.current_stream().cuda_stream
    s.wait_stream(torch.cuda.current_stream())
    out = torch.empty_like(tq)
    got = decode(tq, tk, tv, tl, causal=True, out=out, return_lse=True, num_splits=3, stream=s)
    s.synchronize()
    assert got[0] is out
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert (torch.cuda.current_device(), s.cuda_stream) in fa_mi355x._WS_BUF
    with torch.cuda.stream(s):
        assert dr.ws_counters_zero()
