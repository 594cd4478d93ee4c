"""GPU tests of decode attention over an FP8 (E4M3) K/V cache, contiguous and
paged (fa_decode_kv8_* / fa_decode_paged_kv8_*: Q dtype in {fp16, bf16} x HDIM
in {64, 128} x NB in {1, 2, 4} x {contiguous, paged} = 24 kernels).

The references see the DEQUANTISED cache (K8.float() * k_scale), so the 3-bit
mantissa of E4M3 is not in the comparison and the gates are the project's own
(helpers of tests/decode_refs.py), no new tolerance:
  * fp16 O: the CPU oracle, 1e-3.
  * bf16 O: fp32 torch on the same inputs, 5e-3.
  * LSE: float64 reference, 2^-10 * max|scaled score| + 1e-5.
  * a row that sees no key: O exactly zero, LSE exactly -inf.
The oracle generator draws values in [-0.5, 0.5]; with power-of-two scales
between 2^-8 and 2^-3 no code passes 448 and the dequantised values are exact
in fp16 and in bf16 (both asserted in _case8), so the CPU oracle takes them as
fp16 bits.  Rows past each length hold the byte 0x7f (the E4M3 NaN).  Each K/V
head has its own scales: a kernel that applies head 0's everywhere fails.
"""
import numpy as np
import pytest
import torch

import decode_refs as dr
import fa_mi355x

pytestmark = pytest.mark.gpu

DEV = "cuda"
FP8 = torch.float8_e4m3fn
PAD8 = 0x7f  # the E4M3 NaN
K_SCALE = (2.0 ** -6, 2.0 ** -3)
V_SCALE = (2.0 ** -4, 2.0 ** -8)

decode = fa_mi355x.flash_attention_decode
decode_paged = fa_mi355x.flash_attention_decode_paged


def _scale_t(vals):
    return torch.tensor(list(vals), dtype=torch.float32, device=DEV)


def _quant(x, scale):
    """(E4M3 cache, its fp32 dequantisation) of a [B][Hkv][cap][D] fp32 tensor
    with one scale per K/V head; no code may pass 448."""
    s = _scale_t(scale)[None, :, None, None]
    y = x / s
    assert float(y.abs().max()) <= 448.0
    x8 = y.to(FP8)
    assert bool(torch.isfinite(x8.float()).all())
    return x8, x8.float() * s


def _pad8(x8, lens):
    for i, n in enumerate(lens):
        x8[i, :, int(n):].view(torch.uint8).fill_(PAD8)
    return x8


def _case8(b, hq, hkv, sq, cap, d, lens, dtype, k_scale=K_SCALE, v_scale=V_SCALE, exact=True):
    """The oracle generator's inputs with K and V quantised to E4M3.
    host: (q, dequantised k, dequantised v) as uint16 fp16 bits (exact=True);
    dev:  (q, dequantised k, dequantised v) device tensors, q of `dtype`, k / v of
          `dtype` (exact=True: a lossless cast, asserted) or fp32;
    q8:   (q, k8, v8) for the entry, the caches' rows past each length 0x7f."""
    q, k, v = dr.inputs(b, hq, hkv, sq, cap, d)
    tq = dr.dev(q).to(dtype)
    k8, kd = _quant(dr.dev(k).float(), k_scale)
    v8, vd = _quant(dr.dev(v).float(), v_scale)
    host = None
    if exact:
        for x in (kd, vd):  # the dequantised values are exact in fp16 and in bf16
            assert torch.equal(x.to(torch.float16).float(), x)
            assert torch.equal(x.to(torch.bfloat16).float(), x)
        host = (q, dr.bits(kd.to(torch.float16)), dr.bits(vd.to(torch.float16)))
        kd, vd = kd.to(dtype), vd.to(dtype)
    return host, (tq, kd, vd), (tq, _pad8(k8, lens), _pad8(v8, lens))


def _paginate8(k8, v8, page_size, lens, **kw):
    """dr.paginate on the caches' bytes: FP8 pools whose unused pages and rows
    past each length are 0xff / 0x7f (both NaN in E4M3)."""
    kp, vp, table = dr.paginate(k8.view(torch.uint8), v8.view(torch.uint8), page_size, lens, **kw)
    return kp.view(FP8), vp.view(FP8), table


def _gather8(pages, table):
    return dr.gather(pages.view(torch.uint8), table).view(FP8)


# ---- 1. every variant, split and unsplit --------------------------------------------

MATRIX_LENS = (70, 300, 640)


@pytest.mark.parametrize("g,sq", [(5, 1), (7, 3), (4, 16), (16, 5)])
@pytest.mark.parametrize("d", [128, 64])
@pytest.mark.parametrize("dtype", dr.DTYPES)
def test_variant_split_matrix(dtype, d, g, sq):
    """The shapes of test_decode_matrix_gpu.test_variant_split_matrix: 5 / 21 /
    64 / 80 rows per K/V head (NB = 1 / 2 / 4 / 4 with a second row group), the
    contiguous entry causal and not at num_splits 1, 2, 3, 7 and the paged one
    (pages of 128) causal at 1 and 3: all 24 kv8 kernels, split and unsplit."""
    b, hkv, cap = 3, 2, 640
    lens = np.array(MATRIX_LENS)
    host, dev, (tq, k8, v8) = _case8(b, hkv * g, hkv, sq, cap, d, lens, dtype)
    ks, vs = _scale_t(K_SCALE), _scale_t(V_SCALE)
    tl = dr.lens(lens)
    tag = f"kv8 {dr.name(dtype)} d={d} NB={dr.nb(g, sq)} G={g} Sq={sq}"
    refs = {}
    for causal in (True, False):
        refs[causal] = dr.refs(host, dev, lens, causal, dtype)
        for ns in (1, 2, 3, 7):
            out, lse = decode(tq, k8, v8, tl, causal=causal, return_lse=True, num_splits=ns,
                              k_scale=ks, v_scale=vs)
            dr.check(out, lse, refs[causal], dtype, f"contig {tag} causal={causal} ns={ns}")
            if ns > 1:
                assert dr.ws_counters_zero(), (tag, causal, ns)
    kp, vp, table = _paginate8(k8, v8, 128, lens)
    for ns in (1, 3):
        out, lse = decode_paged(tq, kp, vp, table, tl, causal=True, return_lse=True, num_splits=ns,
                                k_scale=ks, v_scale=vs)
        dr.check(out, lse, refs[True], dtype, f"paged {tag} causal=True ns={ns}")
        if ns > 1:
            assert dr.ws_counters_zero(), (tag, "paged", ns)


# ---- 2. scales that are no powers of two --------------------------------------------

@pytest.mark.parametrize("g,sq,d", [(5, 1, 64), (4, 16, 128)], ids=["NB1", "NB4"])
@pytest.mark.parametrize("dtype", dr.DTYPES)
def test_scales_not_powers_of_two(dtype, g, sq, d):
    """The dequantised cache is then no 16-bit tensor: the reference is fp32
    torch on K8.float() * k_scale, the gate the dtype's own."""
    b, hkv, cap = 2, 2, 320
    lens = np.array([300, 131])
    ksc, vsc = (0.0371, 0.0519), (1.73, 0.613)
    _, dev, (tq, k8, v8) = _case8(b, hkv * g, hkv, sq, cap, d, lens, dtype, ksc, vsc, exact=False)
    assert dev[1].dtype is torch.float32
    refs = dr.refs(None, dev, lens, True, dtype)
    for ns in (1, 3):
        for entry in ("contig", "paged"):
            if entry == "contig":
                out, lse = decode(tq, k8, v8, dr.lens(lens), causal=True, return_lse=True, num_splits=ns,
                                  k_scale=_scale_t(ksc), v_scale=_scale_t(vsc))
            else:
                kp, vp, table = _paginate8(k8, v8, 64, lens, seed=4)
                out, lse = decode_paged(tq, kp, vp, table, dr.lens(lens), causal=True, return_lse=True,
                                        num_splits=ns, k_scale=_scale_t(ksc), v_scale=_scale_t(vsc))
            dr.check(out, lse, refs, dtype, f"{entry} kv8 odd scales {dr.name(dtype)} d={d} G={g} Sq={sq} ns={ns}")


# ---- 3. paged == contiguous, bit for bit ---------------------------------------------

@pytest.mark.parametrize("page_size", [64, 128, 192])
@pytest.mark.parametrize("d", [128, 64])
def test_paged_bit_identical_to_contiguous(d, page_size):
    """The paged kv8 entry on a permuted pool against the contiguous kv8 entry
    on the gathered cache (NaN bytes past each length in both): equal bits."""
    b, hkv, g, sq, cap = 3, 2, 7, 3, 384
    lens = np.array([70, 300, 384])
    _, _, (tq, k8, v8) = _case8(b, hkv * g, hkv, sq, cap, d, lens, torch.bfloat16)
    ks, vs = _scale_t(K_SCALE), _scale_t(V_SCALE)
    kp, vp, table = _paginate8(k8, v8, page_size, lens, seed=page_size)
    gk, gv = _gather8(kp, table), _gather8(vp, table)
    assert gk.shape == k8.shape
    for i, n in enumerate(lens):  # the table describes this cache
        assert torch.equal(gk[i, :, :n].view(torch.uint8), k8[i, :, :n].view(torch.uint8))
    for ns in (1, 3):
        want = decode(tq, gk, gv, dr.lens(lens), causal=True, return_lse=True, num_splits=ns,
                      k_scale=ks, v_scale=vs)
        got = decode_paged(tq, kp, vp, table, dr.lens(lens), causal=True, return_lse=True, num_splits=ns,
                           k_scale=ks, v_scale=vs)
        assert dr.same(got, want), (d, page_size, ns)
        assert bool(torch.isfinite(got[0]).all())


# ---- 4. no scales = scales of one ---------------------------------------------------

@pytest.mark.parametrize("dtype", dr.DTYPES)
def test_none_scales_equal_ones(dtype):
    b, hkv, g, sq, cap, d = 2, 2, 4, 2, 320, 128
    lens = np.array([320, 77])
    one = (1.0, 1.0)
    _, _, (tq, k8, v8) = _case8(b, hkv * g, hkv, sq, cap, d, lens, dtype, one, one)
    ones = _scale_t(one)
    kp, vp, table = _paginate8(k8, v8, 64, lens, seed=9)
    for ns in (1, 2):
        want = decode(tq, k8, v8, dr.lens(lens), return_lse=True, num_splits=ns, k_scale=ones, v_scale=ones)
        assert dr.same(decode(tq, k8, v8, dr.lens(lens), return_lse=True, num_splits=ns), want)
        assert dr.same(decode(tq, k8, v8, dr.lens(lens), return_lse=True, num_splits=ns, v_scale=ones), want)
        pwant = decode_paged(tq, kp, vp, table, dr.lens(lens), return_lse=True, num_splits=ns,
                             k_scale=ones, v_scale=ones)
        assert dr.same(decode_paged(tq, kp, vp, table, dr.lens(lens), return_lse=True, num_splits=ns), pwant)
        assert dr.same(pwant, want)


# ---- 5. short rows and rows that see nothing ----------------------------------------

UNSEEN = [
    (16, 70),   # tile 1 is masked for rows t < 10, live for the rest: -inf beside finite LSEs
    (16, 16),   # rows see 1 .. 16 keys
    (16, 17),   # rows see 2 .. 17 keys
    (5, 3),     # two rows see nothing in any piece; with 2 pieces piece 0 has no tile
    (16, 129),  # three tiles; the last holds one key that only the last row sees
    (1, 1),     # one key
]


@pytest.mark.parametrize("sq,n", UNSEEN)
@pytest.mark.parametrize("dtype", dr.DTYPES)
def test_short_and_unseen_rows(dtype, sq, n):
    lens = np.array([n])
    host, dev, (tq, k8, v8) = _case8(1, 2, 1, sq, 192, 128, lens, dtype, K_SCALE[1:], V_SCALE[1:])
    refs = dr.refs(host, dev, lens, True, dtype)
    if (sq, n) == (5, 3):
        assert np.isneginf(refs[1][:, :, :2]).all() and np.isfinite(refs[1][:, :, 2:]).all()
    ks, vs = _scale_t(K_SCALE[1:]), _scale_t(V_SCALE[1:])
    for ns in (1, 2, 3):
        out, lse = decode(tq, k8, v8, dr.lens(lens), causal=True, return_lse=True, num_splits=ns,
                          k_scale=ks, v_scale=vs)
        dr.check(out, lse, refs, dtype, f"kv8 short {dr.name(dtype)} Sq={sq} len={n} ns={ns}")
        if ns > 1:
            assert dr.ws_counters_zero(), (sq, n, ns)


def test_zero_lengths():
    """Elements with no key at all beside a live one: exactly 0 and -inf."""
    lens = np.array([0, 130, 0])
    _, _, (tq, k8, v8) = _case8(3, 8, 2, 2, 192, 64, lens, torch.float16)
    for ns in (1, 3):
        out, lse = decode(tq, k8, v8, dr.lens(lens), return_lse=True, num_splits=ns,
                          k_scale=_scale_t(K_SCALE), v_scale=_scale_t(V_SCALE))
        for bi in (0, 2):
            assert int(torch.count_nonzero(out[bi]).item()) == 0
            assert bool(torch.isneginf(lse[bi]).all())
        assert bool(torch.isfinite(lse[1]).all()) and bool(torch.isfinite(out).all())


# ---- 6. pool guards -----------------------------------------------------------------

@pytest.mark.parametrize("splits", [1, 3])
def test_nan_pages_and_junk_entries_never_read(splits):
    """Unused pages and the rows past each length are NaN bytes; table entries
    past each length are arbitrary ids (out-of-pool ones among them)."""
    lens = (0, 129, 700, 1)
    _, _, (tq, k8, v8) = _case8(4, 8, 2, 2, 768, 128, lens, torch.float16)
    ks, vs = _scale_t(K_SCALE), _scale_t(V_SCALE)
    tl = dr.lens(lens)
    kp, vp, zeros = _paginate8(k8, v8, 128, lens, seed=5, filler=0)
    kp2, vp2, junk = _paginate8(k8, v8, 128, lens, seed=5, filler="junk")
    assert torch.equal(kp.view(torch.uint8), kp2.view(torch.uint8)) and not torch.equal(zeros, junk)
    used = set(zeros[i, j].item() for i, n in enumerate(lens) for j in range(-(-n // 128)))
    spare = sorted(set(range(kp.shape[0])) - used)
    assert spare and bool(torch.isnan(kp[spare].float()).all())
    want = decode(tq, k8, v8, tl, causal=True, return_lse=True, num_splits=splits, k_scale=ks, v_scale=vs)
    for table in (zeros, junk):
        got = decode_paged(tq, kp, vp, table, tl, causal=True, return_lse=True, num_splits=splits,
                           k_scale=ks, v_scale=vs)
        assert bool(torch.isfinite(got[0]).all())
        assert dr.same(got, want)


@pytest.mark.parametrize("splits", [1, 3])
def test_out_of_range_page_ids_read_as_zero_rows(splits):
    """Ids -2, -1, num_pages, num_pages + 1 and INT_MAX in entries that ARE
    read give the bits of a table that names an all-zero page there.  The pool
    is a slice of a larger NaN-filled allocation, two pages in from either end,
    so even a missing clamp reads only this test's memory -- and then NaN."""
    lens = (200, 320, 129)
    _, _, (tq, k8, v8) = _case8(3, 8, 2, 1, 320, 128, lens, torch.float16)
    ks, vs = _scale_t(K_SCALE), _scale_t(V_SCALE)
    tl = dr.lens(lens)
    kp0, vp0, table = _paginate8(k8, v8, 64, lens, seed=6)
    n = kp0.shape[0]
    zero_page = sorted(set(range(n)) - set(table.flatten().tolist()) - {0})[0]
    bigk = torch.full((n + 4,) + tuple(kp0.shape[1:]), 0xff, dtype=torch.uint8, device=DEV)
    bigv = bigk.clone()
    kp, vp = bigk[2:2 + n], bigv[2:2 + n]
    kp.copy_(kp0.view(torch.uint8))
    vp.copy_(vp0.view(torch.uint8))
    kp[zero_page] = 0
    vp[zero_page] = 0
    kp, vp = kp.view(FP8), vp.view(FP8)
    assert kp.is_contiguous() and vp.is_contiguous()
    zeroed, bad = table.clone(), table.clone()
    for j, pid in zip(range(5), (-2, -1, n, n + 1, 2 ** 31 - 1)):  # element 1 reads entries 0..4
        zeroed[1, j] = zero_page
        bad[1, j] = pid
    want = decode_paged(tq, kp, vp, zeroed, tl, causal=True, return_lse=True, num_splits=splits,
                        k_scale=ks, v_scale=vs)
    got = decode_paged(tq, kp, vp, bad, tl, causal=True, return_lse=True, num_splits=splits,
                       k_scale=ks, v_scale=vs)
    assert bool(torch.isfinite(got[0]).all()) and bool(torch.isfinite(got[1]).all())
    assert dr.same(got, want)
    # all five tiles of element 1 are zero rows: O = 0, LSE = log(320)
    assert int(torch.count_nonzero(got[0][1]).item()) == 0
    assert float((got[1][1] - float(np.log(320.0))).abs().max()) <= 1e-5


# ---- 7. the torch ops, graph capture, streams ---------------------------------------

def test_torch_ops_match_python_entries():
    import fa_mi355x.torch_op  # noqa: F401

    lens = np.array([300, 640])
    _, _, (tq, k8, v8) = _case8(2, 8, 2, 3, 640, 128, lens, torch.bfloat16)
    ks, vs = _scale_t(K_SCALE), _scale_t(V_SCALE)
    tl = dr.lens(lens)
    kp, vp, table = _paginate8(k8, v8, 128, lens, seed=2)
    for causal in (True, False):
        want = decode(tq, k8, v8, tl, causal=causal, k_scale=ks, v_scale=vs)
        assert torch.equal(torch.ops.fa_mi355x.decode(tq, k8, v8, tl, causal, ks, vs), want)
        assert torch.equal(torch.ops.fa_mi355x.decode(tq, k8, v8, tl, causal=causal, k_scale=ks,
                                                      v_scale=vs), want)
        assert torch.equal(torch.ops.fa_mi355x.decode_paged(tq, kp, vp, table, tl, causal, ks, vs), want)
        assert torch.equal(torch.ops.fa_mi355x.decode_paged(tq, kp, vp, table, tl, causal=causal,
                                                            k_scale=ks, v_scale=vs), want)
    plain = decode(tq, k8, v8, tl, causal=True)
    assert not torch.equal(plain, decode(tq, k8, v8, tl, causal=True, k_scale=ks, v_scale=vs))
    assert torch.equal(torch.ops.fa_mi355x.decode(tq, k8, v8, tl, True), plain)
    assert torch.equal(torch.ops.fa_mi355x.decode_paged(tq, kp, vp, table, tl, True), plain)


def test_wrapper_rejects_host_scales():
    lens = np.array([64])
    _, _, (tq, k8, v8) = _case8(1, 2, 2, 1, 64, 64, lens, torch.float16)
    with pytest.raises(fa_mi355x.FlashAttentionError, match="k_scale must be a tensor on"):
        decode(tq, k8, v8, dr.lens(lens), k_scale=torch.ones(2))
    with pytest.raises(fa_mi355x.FlashAttentionError, match="go with a torch.float8_e4m3fn cache only"):
        decode(tq, k8.to(torch.float16), v8.to(torch.float16), dr.lens(lens), k_scale=_scale_t((1.0, 1.0)))


def test_op_in_hip_graph_follows_lengths_and_scales():
    """One capture, two replays; before each, kv_lens and both scale tensors
    are rewritten in place (the cache's bytes stay): each replay gives the
    eager result of the values it finds."""
    import fa_mi355x.torch_op  # noqa: F401

    op = torch.ops.fa_mi355x.decode
    _, _, (tq, k8, v8) = _case8(1, 8, 2, 1, 2048, 128, np.array([2048]), torch.float16)
    lens = dr.lens([2048])
    ks, vs = _scale_t(K_SCALE), _scale_t(V_SCALE)
    settings = [(700, (2.0 ** -5, 2.0 ** -7), (0.75, 2.0 ** -3)), (1333, (0.011, 2.0 ** -4), (2.0 ** -6, 1.5))]
    wants = []
    for n, a, bb in [(2048, K_SCALE, V_SCALE)] + settings:  # eager references, outside the capture
        lens.fill_(n)
        ks.copy_(_scale_t(a))
        vs.copy_(_scale_t(bb))
        wants.append(op(tq, k8, v8, lens, True, ks, vs).clone())
    assert not torch.equal(wants[1], wants[2]) and not torch.equal(wants[0], wants[1])
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        op(tq, k8, v8, lens, True, ks, vs)  # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = op(tq, k8, v8, lens, True, ks, vs)
    for (n, a, bb), want in zip(settings, wants[1:]):
        lens.fill_(n)
        ks.copy_(_scale_t(a))
        vs.copy_(_scale_t(bb))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, want), n


def test_non_default_stream():
    """stream= another stream: the default stream's bits, its counters back to zero."""
    b, hkv, g, sq, cap, d = 3, 2, 7, 3, 640, 128
    lens = np.array(MATRIX_LENS)
    _, _, (tq, k8, v8) = _case8(b, hkv * g, hkv, sq, cap, d, lens, torch.float16)
    ks, vs = _scale_t(K_SCALE), _scale_t(V_SCALE)
    tl = dr.lens(lens)
    want = decode(tq, k8, v8, tl, causal=True, return_lse=True, num_splits=3, k_scale=ks, v_scale=vs)
    s = torch.cuda.Stream()
    assert s.cuda_stream != torch.cuda.current_stream().cuda_stream
    s.wait_stream(torch.cuda.current_stream())
    out = torch.empty_like(tq)
    got = decode(tq, k8, v8, tl, causal=True, out=out, return_lse=True, num_splits=3, stream=s,
                 k_scale=ks, v_scale=vs)
    s.synchronize()
    assert got[0] is out and dr.same(got, want)
    with torch.cuda.stream(s):
        assert dr.ws_counters_zero()


# ---- 8. informational: what the quantisation itself costs on this data --------------

@pytest.mark.parametrize("dtype", dr.DTYPES)
def test_report_quantisation_error(dtype):
    """Printed, not gated: kv8 output against the 16-bit entry on the
    UNQUANTISED cache at len 640 (the error of E4M3's 3-bit mantissa on the
    oracle generator's data, not the kernel's)."""
    b, hkv, g, sq, cap, d = 1, 2, 4, 1, 640, 128
    lens = np.array([640])
    q, k, v = dr.inputs(b, hkv * g, hkv, sq, cap, d)
    _, _, (tq, k8, v8) = _case8(b, hkv * g, hkv, sq, cap, d, lens, dtype)
    ref = decode(tq, dr.dev(k).to(dtype), dr.dev(v).to(dtype), dr.lens(lens), causal=True)
    got = decode(tq, k8, v8, dr.lens(lens), causal=True, k_scale=_scale_t(K_SCALE), v_scale=_scale_t(V_SCALE))
    err = float((got.float() - ref.float()).abs().max())
    print(f"kv8 vs 16-bit cache, {dr.name(dtype)} d={d} len=640: max_abs_diff {err:.3e} "
          f"(max |O| {float(ref.float().abs().max()):.3e})")
    assert bool(torch.isfinite(got).all())
