"""GPU tests of the fused RoPE + cache append (fa_rope_append_* behind
fa_mi355x.flash_attention_rope_append[_varlen][_paged] and the torch ops).

Every comparison is bit-exact; the feature has no tolerance.  The caches and
q_out are compared whole, as integers, with an expectation built on the CPU
(tests/rope_refs.py: the contract's torch expression, then torch indexing)
over a sentinel fill, so one assertion checks the written rows and that every
other byte is untouched.  FP8 bytes come from the CPU reference of
tests/fp8_contract.py applied to the CPU-rotated 16-bit K.
Shapes are the append tests': B = 3, Hkv = 2 (one Hkv = 1 case), cap = 192;
paged: page 64, a 3-column table into a permuted pool with two pages no entry
names.  Inputs are randn with a few exact zeros and negative zeros (the
contract is for finite data).
"""
import pytest
import torch

import fa_mi355x
import rope_refs
from fp8_contract import torch_reference_bytes

pytestmark = pytest.mark.gpu

DEV = "cuda"
FP8 = torch.float8_e4m3fn
CAP, PAGE, COLS = 192, 64, 3
SENT16, SENT8, SENTQ = 0x5a3c, 0x5a, 0x3b6d
ROPE_LEN = 256
F16, BF16 = torch.float16, torch.bfloat16
FORMS = [pytest.param((False, False), id="contig-16"), pytest.param((True, False), id="paged-16"),
         pytest.param((False, True), id="contig-kv8"), pytest.param((True, True), id="paged-kv8")]
# per Sn, the lengths AFTER the append of the three batch elements (the append
# tests' cases: page crossings, len = n, len < n, len = 0, len past cap)
LENS = {1: (1, 0, 192), 3: (65, 2, 197), 16: (70, 16, 192), 67: (67, 197, 30)}
K_SCALE, V_SCALE = (0.25, 0.3), (3.7, 2.0 ** -6)

rope_append = fa_mi355x.flash_attention_rope_append
rope_append_paged = fa_mi355x.flash_attention_rope_append_paged
rope_append_varlen = fa_mi355x.flash_attention_rope_append_varlen
rope_append_varlen_paged = fa_mi355x.flash_attention_rope_append_varlen_paged
append = fa_mi355x.flash_attention_cache_append
append_paged = fa_mi355x.flash_attention_cache_append_paged


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _i32(vals):
    return torch.tensor(list(vals), dtype=torch.int32, device=DEV)


def _randn(shape, dtype, g):
    """randn with a few exact zeros and negative zeros."""
    x = torch.randn(shape, generator=g).to(dtype)
    flat = x.view(-1)
    flat[::97] = 0.0
    flat[5::193] = -0.0
    return x


def _table(b, cols, g, spare=2):
    """A permuted pool: b * cols table entries into b * cols + spare pages."""
    n = b * cols + spare
    perm = torch.randperm(n, generator=g).to(torch.int32)
    return perm[:b * cols].reshape(b, cols).contiguous(), n


def _quantise(x, scales):
    """CPU reference bytes of a [B,Hkv,S,D] 16-bit CPU tensor, one scale per head."""
    return torch.stack([torch_reference_bytes(x[:, h], float(scales[h])) for h in range(x.shape[1])], 1)


def _raw(x):
    return x.view(torch.uint8 if x.element_size() == 1 else torch.int16)


class Case:
    """One problem on the CPU -- inputs, tables, the CPU-rotated Q and K, the
    sentinel-filled caches and q_out and what they must hold afterwards -- and
    fresh device copies of it."""

    def __init__(self, dtype, d, form, interleaved, r, hq, sn, lens, new_lens=None, hkv=2,
                 rope_len=ROPE_LEN, seed=0, bad_ids=False, cap=CAP):
        g = _gen(seed)
        self.paged, self.kv8 = form
        self.dtype, self.interleaved, self.lens, self.new_lens = dtype, interleaved, lens, new_lens
        b = len(lens)
        self.q, self.kn, self.vn = (_randn((b, h, sn, d), dtype, g) for h in (hq, hkv, hkv))
        self.cos, self.sin = rope_refs.rope_tables(rope_len, r)
        self.table, shape = None, (b, hkv, cap, d)
        if self.paged:
            self.table, npages = _table(b, cap // PAGE, g)
            if bad_ids:  # entries the append uses: element 0's column 0, element 1's column 2
                self.table[0, 0] = -1
                self.table[1, 2] = npages
            shape = (npages, hkv, PAGE, d)
        self.q_rot, self.valid = rope_refs.rotate_tokens(self.q, self.cos, self.sin, lens, new_lens, interleaved)
        self.k_rot, _ = rope_refs.rotate_tokens(self.kn, self.cos, self.sin, lens, new_lens, interleaved)
        if self.kv8:
            self.scales = [torch.tensor(s[:hkv], dtype=torch.float32) for s in (K_SCALE, V_SCALE)]
            self.k0 = torch.full(shape, SENT8, dtype=torch.uint8)
            self.v0 = torch.full(shape, SENT8 ^ 0x11, dtype=torch.uint8)
            src_k, src_v = _quantise(self.k_rot, self.scales[0]), _quantise(self.vn, self.scales[1])
        else:
            self.scales = None
            self.k0 = torch.full(shape, SENT16, dtype=torch.int16)
            self.v0 = torch.full(shape, SENT16 ^ 0x0101, dtype=torch.int16)
            src_k, src_v = self.k_rot.view(torch.int16), self.vn.view(torch.int16)
        self.want_k = rope_refs.expect_cache(self.k0, src_k, lens, new_lens, self.table, rope_len)
        self.want_v = rope_refs.expect_cache(self.v0, src_v, lens, new_lens, self.table, rope_len)
        self.q0 = torch.full(self.q.shape, SENTQ, dtype=torch.int16)
        self.want_q = rope_refs.expect_q(self.q0, self.q_rot.view(torch.int16), self.valid)

    def caches(self):
        view = (lambda x: x.view(FP8)) if self.kv8 else (lambda x: x.view(self.dtype))
        return view(self.k0.to(DEV)), view(self.v0.to(DEV))

    def scale_kw(self):
        return dict(k_scale=self.scales[0].to(DEV), v_scale=self.scales[1].to(DEV)) if self.kv8 else {}

    def run(self, q="default", q_out="sentinel", kn=None, fused=True):
        """The fused call (or, fused=False, the existing append of `kn`) on
        fresh caches.  Returns (k cache, v cache, q_out), raw, on the CPU."""
        kc, vc = self.caches()
        kn = (self.kn if kn is None else kn).to(DEV)
        lens = _i32(self.lens)
        new_lens = None if self.new_lens is None else _i32(self.new_lens)
        tab = () if self.table is None else (self.table.to(DEV),)
        out = None
        if fused:
            q = self.q.to(DEV) if isinstance(q, str) else q
            if isinstance(q_out, str):
                q_out = None if q is None else self.q0.to(DEV).view(self.dtype)
            fn = rope_append_paged if self.paged else rope_append
            out = fn(q, kn, self.vn.to(DEV), kc, vc, *tab, lens, self.cos.to(DEV), self.sin.to(DEV), new_lens,
                     self.interleaved, q_out, **self.scale_kw())
            assert q_out is None or out is q_out
        else:
            (append_paged if self.paged else append)(kn, self.vn.to(DEV), kc, vc, *tab, lens, new_lens,
                                                     **self.scale_kw())
        torch.cuda.synchronize()
        return _raw(kc).cpu(), _raw(vc).cpu(), None if out is None else out.view(torch.int16).cpu()

    def check(self, got):
        k, v, q = got
        assert torch.equal(k, self.want_k), "k cache"
        assert torch.equal(v, self.want_v), "v cache"
        assert torch.equal(q, self.want_q), "q_out"


# (dtype, D, interleaved, R, Hq, Sn): every value of every axis -- both types,
# both head dims, both styles, R in {D, D/2, 16} and 96 at D = 128 (a NeoX
# partner distance that is no power of two), Hq in {2, 4, 6}, the four Sn of
# LENS -- appears at least once, and the list runs over each cache form
THIN = [(F16, 128, False, 128, 4, 67), (BF16, 128, False, 96, 6, 16), (F16, 64, False, 32, 2, 3),
        (BF16, 64, True, 64, 4, 67), (F16, 128, True, 64, 6, 1), (BF16, 128, True, 16, 2, 16),
        (BF16, 64, False, 16, 6, 67), (F16, 128, True, 96, 2, 3), (F16, 64, True, 16, 4, 1),
        (BF16, 128, False, 64, 2, 67)]


def _id(c):
    return f"{'bf16' if c[0] is BF16 else 'f16'}-d{c[1]}-{'gptj' if c[2] else 'neox'}-r{c[3]}-hq{c[4]}-sn{c[5]}"


@pytest.mark.parametrize("case", THIN, ids=_id)
@pytest.mark.parametrize("form", FORMS)
def test_whole_cache_and_q_out(form, case):
    dtype, d, inter, r, hq, sn = case
    c = Case(dtype, d, form, inter, r, hq, sn, LENS[sn], seed=sn + d + r)
    c.check(c.run())
    assert bool(c.valid.any()) and not torch.equal(c.want_q, c.q.view(torch.int16))  # something was rotated


@pytest.mark.parametrize("form", [FORMS[0], FORMS[3]])
def test_four_head_slots_per_workgroup(form):
    """A launch of 1024 workgroups or more gives each workgroup four head slots
    (the table rows stay in registers over them): B = 8, Sn = 1024 (16 token
    blocks), Hkv + Hq = 2 + 30 slots make exactly 1024, with K/V and Q slots
    mixed in one workgroup; one slot fewer stays on the one-slot path."""
    lens = (1024, 1030, 1500, 1025, 2000, 1024, 1111, 1999)
    for hq in (30, 26):
        c = Case(F16, 128, form, False, 128, hq, 1024, lens, rope_len=2048, cap=1536, seed=31 + hq)
        c.check(c.run())


@pytest.mark.parametrize("form", FORMS)
def test_one_kv_head_and_odd_query_heads(form):
    """Hkv = 1 with Hq = 3: heads_q need not divide by heads_kv."""
    c = Case(F16, 128, form, False, 128, 3, 16, LENS[16], hkv=1, seed=5)
    c.check(c.run())


@pytest.mark.parametrize("inter", [False, True], ids=["neox", "gptj"])
@pytest.mark.parametrize("form", FORMS)
def test_identity_with_the_existing_append(form, inter):
    """The fused call's caches equal flash_attention_cache_append of the
    CPU-rotated K with the same scales, byte for byte."""
    c = Case(BF16, 128, form, inter, 96, 4, 67, LENS[67], seed=11)
    k, v, _ = c.run()
    k2, v2, _ = c.run(kn=c.k_rot, fused=False)
    assert torch.equal(k, k2) and torch.equal(v, v2)
    assert bool((k != c.k0).any())


@pytest.mark.parametrize("form", FORMS)
def test_new_lens(form):
    """0, 1, Sn, Sn + 4 (clamped to Sn) and -3 (nothing written) in one batch."""
    sn = 16
    c = Case(BF16, 64, form, False, 64, 4, sn, (40, 66, 70, 192, 100), (0, 1, sn, sn + 4, -3), seed=9)
    c.check(c.run())


@pytest.mark.parametrize("form", FORMS)
def test_rope_len_smaller_than_the_lengths(form):
    """rope_len = 100 against lengths up to 197: rows at pos >= 100 are not
    written in K, V or q_out (and no table row past the end is read)."""
    for sn in (3, 67):
        c = Case(F16, 128, form, sn == 3, 64, 4, sn, LENS[sn], rope_len=100, seed=13)
        assert not bool(c.valid.all()) and bool(c.valid.any())
        c.check(c.run())


@pytest.mark.parametrize("kv8", [False, True], ids=["16", "kv8"])
def test_out_of_pool_page_ids_drop_kv_not_q(kv8):
    c = Case(F16, 128, (True, kv8), False, 128, 4, 67, (67, 192, 130), seed=6, bad_ids=True)
    good = Case(F16, 128, (True, kv8), False, 128, 4, 67, (67, 192, 130), seed=6)
    assert not torch.equal(c.want_k, good.want_k)       # the dropped rows were in use
    assert torch.equal(c.want_q, good.want_q) and bool(c.valid.all())   # every Q row is written
    c.check(c.run())


@pytest.mark.parametrize("form", FORMS)
def test_in_place_and_no_q(form):
    """q_out = q (in place) equals out of place; q = None gives the fused K/V result."""
    c = Case(F16, 64, form, False, 64, 6, 67, LENS[67], seed=17)
    k, v, q = c.run()
    c.check((k, v, q))
    qin = c.q.to(DEV)
    k2, v2, q2 = c.run(q=qin, q_out=qin)
    # in place: the rows that are not written keep q's own values
    want = torch.where(c.valid[:, None, :, None], c.q_rot.view(torch.int16), c.q.view(torch.int16))
    assert torch.equal(q2, want) and torch.equal(k2, k) and torch.equal(v2, v)
    k3, v3, q3 = c.run(q=None)
    assert q3 is None and torch.equal(k3, k) and torch.equal(v3, v)
    # q_out=None allocates: the written rows are the rotated ones
    _, _, q4 = c.run(q_out=None)
    rows = c.valid[:, None, :, None].expand_as(q4)
    assert torch.equal(q4[rows], c.want_q[rows])


@pytest.mark.parametrize("form", FORMS)
def test_packed_equals_padded(form):
    """Three ragged sequences, a zero-length one among them, packed between
    rows that belong to none: caches and the unpacked q_out equal the padded
    call's, and the rows outside cu keep the sentinel."""
    n = (37, 0, 67)
    lens = (70, 16, 197)
    c = Case(BF16, 128, form, False, 96, 4, 67, lens, n, seed=19)
    k, v, q = c.run()
    c.check((k, v, q))
    lead, trail = 2, 3
    total = lead + sum(n) + trail
    cu = [lead, lead + n[0], lead + n[0] + n[1], lead + sum(n)]

    def pack(x, fill):
        out = torch.full((total, x.shape[1], x.shape[3]), fill, dtype=torch.int16).view(x.dtype)
        for b in range(3):
            out[cu[b]:cu[b + 1]] = x[b, :, :n[b]].transpose(0, 1)
        return out

    qp, kp, vp = pack(c.q, 0x3c00), pack(c.kn, 0x3c00), pack(c.vn, 0x3c00)
    kc, vc = c.caches()
    qo = torch.full(qp.shape, SENTQ, dtype=torch.int16, device=DEV).view(c.dtype)
    fn = rope_append_varlen_paged if c.paged else rope_append_varlen
    tab = (c.table.to(DEV),) if c.paged else ()
    out = fn(qp.to(DEV), kp.to(DEV), vp.to(DEV), kc, vc, *tab, _i32(cu), _i32(lens), c.cos.to(DEV),
             c.sin.to(DEV), c.interleaved, qo, **c.scale_kw())
    torch.cuda.synchronize()
    assert out is qo
    assert torch.equal(_raw(kc).cpu(), k) and torch.equal(_raw(vc).cpu(), v)
    got = qo.view(torch.int16).cpu()
    want = torch.full(qp.shape, SENTQ, dtype=torch.int16)
    for b in range(3):
        want[cu[b]:cu[b + 1]] = q[b, :, :n[b]].transpose(0, 1)
    assert torch.equal(got, want)
    assert bool((got[:lead] == SENTQ).all()) and bool((got[cu[3]:] == SENTQ).all())


@pytest.mark.parametrize("form", FORMS)
def test_torch_ops_equal_python_functions(form):
    import fa_mi355x.torch_op  # noqa: F401

    ops = torch.ops.fa_mi355x
    c = Case(F16, 64, form, True, 32, 4, 16, LENS[16], (16, 3, 0), seed=10)
    k, v, q = c.run()
    c.check((k, v, q))
    rows = c.valid[:, None, :, None].expand_as(q)
    kc, vc = c.caches()
    tab = (c.table.to(DEV),) if c.paged else ()
    op = ops.rope_append_paged if c.paged else ops.rope_append
    qin = c.q.to(DEV)
    out = op(qin, c.kn.to(DEV), c.vn.to(DEV), kc, vc, *tab, _i32(c.lens), c.cos.to(DEV), c.sin.to(DEV),
             _i32(c.new_lens), True, **c.scale_kw())
    torch.cuda.synchronize()
    assert out.data_ptr() != qin.data_ptr() and out.shape == qin.shape and out.dtype == qin.dtype
    assert torch.equal(_raw(kc).cpu(), k) and torch.equal(_raw(vc).cpu(), v)
    assert torch.equal(out.view(torch.int16).cpu()[rows], q[rows])
    # the packed ops, on the same tokens
    n = [16, 3, 0]
    cu = [0, 16, 19, 19]
    pack = lambda x: torch.cat([x[b, :, :n[b]].transpose(0, 1) for b in range(3)]).contiguous()  # noqa: E731
    kc, vc = c.caches()
    op = ops.rope_append_varlen_paged if c.paged else ops.rope_append_varlen
    out = op(pack(c.q).to(DEV), pack(c.kn).to(DEV), pack(c.vn).to(DEV), kc, vc, *tab, _i32(cu), _i32(c.lens),
             c.cos.to(DEV), c.sin.to(DEV), True, **c.scale_kw())
    torch.cuda.synchronize()
    assert torch.equal(_raw(kc).cpu(), k) and torch.equal(_raw(vc).cpu(), v)
    assert torch.equal(out.view(torch.int16).cpu(), pack(q))


def test_graph_capture_rope_append_then_decode():
    """rope_append + decode captured in one graph; kv_lens (+1) and the new
    tokens are rewritten in place between replays and each replay equals the
    eager pair on a copy of the cache."""
    g = _gen(8)
    b, hq, hkv, d = 3, 4, 2, 128
    dtype = BF16
    cos, sin = (t.to(DEV) for t in rope_refs.rope_tables(ROPE_LEN, d))
    kc = (torch.randn((b, hkv, CAP, d), generator=g) * 0.5).to(dtype).to(DEV)
    vc = kc.clone()
    q, kn, vn = (torch.zeros((b, h, 1, d), dtype=dtype, device=DEV) for h in (hq, hkv, hkv))
    lens = _i32([10, 63, 130])

    def pair(kcache, vcache):
        qr = rope_append(q, kn, vn, kcache, vcache, lens, cos, sin)
        return fa_mi355x.flash_attention_decode(qr, kcache, vcache, lens, num_splits=1)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        pair(kc, vc)  # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = pair(kc, vc)
    prev = None
    for step in range(3):
        for t in (q, kn, vn):
            t.copy_((torch.randn(t.shape, generator=g) * 0.5).to(dtype))
        lens.add_(1)
        kcopy, vcopy = kc.clone(), vc.clone()
        want = pair(kcopy, vcopy).clone()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out.view(torch.int16), want.view(torch.int16)), step
        assert torch.equal(_raw(kc), _raw(kcopy)) and torch.equal(_raw(vc), _raw(vcopy))
        assert prev is None or not torch.equal(prev, want)
        prev = want


def test_chain_rope_append_then_prefill():
    """rope_append then flash_attention_prefill equals the existing append of
    the CPU-rotated K then prefill on the same CPU-rotated Q, bit for bit."""
    sn, lens = 67, (67, 150, 100)
    c = Case(F16, 128, (False, False), False, 128, 4, sn, lens, seed=23)
    assert bool(c.valid.all())
    prefill = fa_mi355x.flash_attention_prefill
    outs = []
    for fused in (True, False):
        g = _gen(29)
        kc = (torch.randn((3, 2, CAP, 128), generator=g) * 0.5).to(F16).to(DEV)
        vc = kc.clone()
        dl = _i32(lens)
        if fused:
            qr = rope_append(c.q.to(DEV), c.kn.to(DEV), c.vn.to(DEV), kc, vc, dl, c.cos.to(DEV), c.sin.to(DEV))
        else:
            append(c.k_rot.to(DEV), c.vn.to(DEV), kc, vc, dl)
            qr = c.q_rot.to(DEV)
        o, lse = prefill(qr, kc, vc, dl, return_lse=True)
        torch.cuda.synchronize()
        outs.append((o.view(torch.int16).cpu(), lse.view(torch.int32).cpu(), _raw(kc).cpu()))
    for a, b in zip(*outs):
        assert torch.equal(a, b)
